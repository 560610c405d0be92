/*
 * edt_api.hip -- C-ABI of the distance map and the surface distances (include/sift3d.h, "exact Euclidean distance map"; DESIGN.md
 * section 7l): sift3d_distance_map and the stage sift3d_surface_distances.  The kernels are in kernels_edt.hip; the defaults, the
 * voxel size and the figures of a label from its two lists are host arithmetic (edt_host.c), the label check and the voxel counts
 * the fusion's (fuse_host.c).
 */
#include <cstring>
#include <vector>

#include "device_call.h"

hipError_t sift3d_launch_edt_surface(hipStream_t s, const unsigned short *lab_a, const unsigned long long *valid_a, const unsigned short *lab_b,
                                     const unsigned long long *valid_b, int64_t nx, int64_t ny, int64_t nz, unsigned l, unsigned char *sites_a,
                                     unsigned char *sites_b, unsigned *counts);
hipError_t sift3d_launch_edt_x(hipStream_t s, const unsigned char *sites, int64_t nx, int64_t ny, int64_t nz, unsigned short *dx);
hipError_t sift3d_launch_edt_line(hipStream_t s, int axis, const void *in, unsigned long long *out, int64_t nx, int64_t ny, int64_t nz, unsigned s_x,
                                  unsigned s_axis);
hipError_t sift3d_launch_edt_gather(hipStream_t s, const unsigned char *at, const unsigned long long *d2, int64_t n, unsigned cap, unsigned *cursor,
                                    unsigned long long *list);

/* SIFT3D_OK, or SIFT3D_ERR_ARG and which argument the transform refuses */
static int check_map(int64_t nx, int64_t ny, int64_t nz, const uint32_t spacing_um[3], char *err, int64_t err_len)
{
    const int64_t ext[3] = {nx, ny, nz};
    const char *axis[3] = {"nx", "ny", "nz"};
    if (!spacing_um) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    for (int c = 0; c < 3; c++)
        if (ext[c] < 1 || ext[c] > SIFT3D_EDT_MAX_EXTENT)
            return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s = %lld: an extent must be 1 .. %d", axis[c], (long long)ext[c], SIFT3D_EDT_MAX_EXTENT);
    if (nx * ny * nz > SIFT3D_EDT_MAX_VOXELS)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "nx ny nz = %lld: more than 2^30 voxels", (long long)(nx * ny * nz));
    for (int c = 0; c < 3; c++)
        if (spacing_um[c] < 1 || spacing_um[c] > SIFT3D_EDT_MAX_SPACING_UM)
            return call_fail(err, err_len, SIFT3D_ERR_ARG, "spacing_um[%d] = %u: a spacing must be 1 .. %u micrometres", c, (unsigned)spacing_um[c],
                             SIFT3D_EDT_MAX_SPACING_UM);
    return SIFT3D_OK;
}

/* the four events around the three passes of one transform */
typedef stage_events<4> edt_events;

/* total, x, y, z into ms[0 .. 3]; the stream has been synchronised */
static hipError_t edt_elapsed(const edt_events &ev, double ms[4])
{
    const int from[4] = {0, 0, 1, 2}, to[4] = {3, 1, 2, 3};
    hipError_t rc = hipSuccess;
    for (int i = 0; i < 4 && rc == hipSuccess; i++) rc = ev.elapsed(from[i], to[i], &ms[i]);
    return rc;
}

/* sites to d2 through the uint16 plane dx and the 64-bit plane tmp */
static hipError_t run_map(hipStream_t s, const unsigned char *sites, int64_t nx, int64_t ny, int64_t nz, const uint32_t sp[3], unsigned short *dx,
                          unsigned long long *tmp, unsigned long long *d2, const edt_events &ev)
{
    hipError_t rc = ev.record(0, s);
    if (rc == hipSuccess) rc = sift3d_launch_edt_x(s, sites, nx, ny, nz, dx);
    if (rc == hipSuccess) rc = ev.record(1, s);
    if (rc == hipSuccess) rc = sift3d_launch_edt_line(s, 1, dx, tmp, nx, ny, nz, sp[0], sp[1]);
    if (rc == hipSuccess) rc = ev.record(2, s);
    if (rc == hipSuccess) rc = sift3d_launch_edt_line(s, 2, tmp, d2, nx, ny, nz, sp[0], sp[2]);
    if (rc == hipSuccess) rc = ev.record(3, s);
    return rc;
}

extern "C" int sift3d_distance_map(int device, const uint8_t *sites, int64_t nx, int64_t ny, int64_t nz, const uint32_t spacing_um[3], uint64_t *d2,
                                   double kernel_ms[4], char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = kernel_ms[3] = 0.0;
    if (!sites || !d2) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    const int bad = check_map(nx, ny, nz, spacing_um, err, err_len);
    if (bad != SIFT3D_OK) return bad;
    const size_t nv = (size_t)(nx * ny * nz);
    device_call dc(err, err_len);
    edt_events ev;
    unsigned char *d_sites;
    unsigned short *d_dx;
    unsigned long long *d_tmp, *d_d2;
    DEVCHK(dc, dc.open(device, false));
    DEVCHK(dc, ev.create());
    if (dc.alloc(&d_sites, nv) != hipSuccess || dc.alloc(&d_dx, nv) != hipSuccess || dc.alloc(&d_tmp, nv) != hipSuccess || dc.alloc(&d_d2, nv) != hipSuccess)
        return dc.no_memory();
    DEVCHK(dc, dc.to_device(d_sites, (const unsigned char *)sites, nv));
    DEVCHK(dc, run_map(dc.s, d_sites, nx, ny, nz, spacing_um, d_dx, d_tmp, d_d2, ev));
    DEVCHK(dc, dc.download((unsigned long long *)d2, d_d2, nv));
    DEVCHK(dc, dc.sync());
    if (kernel_ms) DEVCHK(dc, edt_elapsed(ev, kernel_ms));
    return SIFT3D_OK;
}

extern "C" int sift3d_surface_distances(const float *a, const float *b, int64_t nx, int64_t ny, int64_t nz, const uint32_t spacing_um[3],
                                        const sift3d_surface_params *pp, sift3d_surface_record *records, int32_t *n_records, double *kernel_ms, char *err,
                                        int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (n_records) *n_records = 0;
    sift3d_surface_params p;
    if (pp) p = *pp;
    else sift3d_surface_defaults(&p);
    if (!a || !b || !records || !n_records) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    const int bad = check_map(nx, ny, nz, spacing_um, err, err_len);
    if (bad != SIFT3D_OK) return bad;
    if (p.first_label < 0 || p.first_label >= SIFT3D_LABEL_COUNT) return call_fail(err, err_len, SIFT3D_ERR_ARG, "first_label = %d: 0 .. 65535", (int)p.first_label);
    if (p.max_labels < 1) return call_fail(err, err_len, SIFT3D_ERR_ARG, "max_labels = %d: at least 1", (int)p.max_labels);
    const int64_t n = nx * ny * nz;
    const float *vols[2] = {a, b};
    std::vector<int64_t> counts(3 * SIFT3D_LABEL_COUNT);
    int64_t *ca = counts.data(), *cb = ca + SIFT3D_LABEL_COUNT;
    if (sift3d_label_overlap(a, b, n, ca, cb, cb + SIFT3D_LABEL_COUNT) < 0) { /* it has checked both volumes: only a refusal looks for the voxel */
        if (check_labels("volume a: ", a, n, err, err_len) != SIFT3D_OK || check_labels("volume b: ", b, n, err, err_len) != SIFT3D_OK)
            return SIFT3D_ERR_ARG;
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the label volumes cannot be counted");
    }
    std::vector<int32_t> labels;
    for (int32_t l = p.first_label; l < SIFT3D_LABEL_COUNT; l++)
        if (ca[l] > 0 || cb[l] > 0) labels.push_back(l);
    if (labels.size() > (size_t)p.max_labels)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "%zu labels from %d on occur in the volumes: more than max_labels = %d", labels.size(), (int)p.first_label,
                         (int)p.max_labels);
    if (labels.empty()) return SIFT3D_OK;

    const size_t nv = (size_t)n, nw = (nv + 63) / 64;
    device_call dc(err, err_len);
    edt_events ev_ab, ev_ba;
    float *d_f;
    unsigned short *d_lab[2], *d_dx;
    unsigned long long *d_valid[2], *d_tmp, *d_d2;
    unsigned char *d_sites[2];
    unsigned *d_cnt; /* the two surface counts and the two gather cursors */
    DEVCHK(dc, dc.open(p.device, false));
    DEVCHK(dc, ev_ab.create());
    DEVCHK(dc, ev_ba.create());
    if (dc.alloc(&d_f, nv) != hipSuccess || dc.alloc(&d_lab[0], nv) != hipSuccess || dc.alloc(&d_lab[1], nv) != hipSuccess ||
        dc.alloc(&d_valid[0], nw) != hipSuccess || dc.alloc(&d_valid[1], nw) != hipSuccess || dc.alloc(&d_sites[0], nv) != hipSuccess ||
        dc.alloc(&d_sites[1], nv) != hipSuccess || dc.alloc(&d_dx, nv) != hipSuccess || dc.alloc(&d_tmp, nv) != hipSuccess || dc.alloc(&d_d2, nv) != hipSuccess ||
        dc.alloc(&d_cnt, 4) != hipSuccess)
        return dc.no_memory();
    for (int v = 0; v < 2; v++) {
        DEVCHK(dc, dc.to_device(d_f, vols[v], nv));
        DEVCHK(dc, sift3d_launch_label_plane(dc.s, d_f, n, d_lab[v], d_valid[v]));
    }
    std::vector<unsigned long long> list_ab, list_ba;
    double total_ms = 0.0;
    for (size_t k = 0; k < labels.size(); k++) {
        sift3d_surface_record &r = records[k];
        memset(&r, 0, sizeof r);
        r.label = labels[k];
        r.voxels_a = ca[labels[k]];
        r.voxels_b = cb[labels[k]];
        unsigned cnt[2] = {0, 0};
        DEVCHK(dc, hipMemsetAsync(d_cnt, 0, 4 * sizeof(unsigned), dc.s));
        DEVCHK(dc, sift3d_launch_edt_surface(dc.s, d_lab[0], d_valid[0], d_lab[1], d_valid[1], nx, ny, nz, (unsigned)labels[k], d_sites[0], d_sites[1], d_cnt));
        DEVCHK(dc, dc.download(cnt, d_cnt, 2));
        DEVCHK(dc, dc.sync());
        if (cnt[0] == 0 || cnt[1] == 0) { /* one volume lacks the label: there is no distance to take */
            sift3d_surface_stats(nullptr, cnt[0], nullptr, cnt[1], &r);
            continue;
        }
        list_ab.resize(cnt[0]);
        list_ba.resize(cnt[1]);
        /* the 64-bit plane between the y and the z pass is free once a map is done: it takes the list */
        DEVCHK(dc, run_map(dc.s, d_sites[1], nx, ny, nz, spacing_um, d_dx, d_tmp, d_d2, ev_ab));
        DEVCHK(dc, sift3d_launch_edt_gather(dc.s, d_sites[0], d_d2, n, cnt[0], d_cnt + 2, d_tmp));
        DEVCHK(dc, dc.download(list_ab.data(), d_tmp, list_ab.size()));
        DEVCHK(dc, run_map(dc.s, d_sites[0], nx, ny, nz, spacing_um, d_dx, d_tmp, d_d2, ev_ba));
        DEVCHK(dc, sift3d_launch_edt_gather(dc.s, d_sites[1], d_d2, n, cnt[1], d_cnt + 3, d_tmp));
        DEVCHK(dc, dc.download(list_ba.data(), d_tmp, list_ba.size()));
        DEVCHK(dc, dc.sync());
        double ms_ab, ms_ba;
        DEVCHK(dc, ev_ab.elapsed(0, 3, &ms_ab));
        DEVCHK(dc, ev_ba.elapsed(0, 3, &ms_ba));
        total_ms += ms_ab;
        total_ms += ms_ba;
        sift3d_surface_stats((uint64_t *)list_ab.data(), cnt[0], (uint64_t *)list_ba.data(), cnt[1], &r);
    }
    *n_records = (int32_t)labels.size();
    if (kernel_ms) *kernel_ms = total_ms;
    return SIFT3D_OK;
}
