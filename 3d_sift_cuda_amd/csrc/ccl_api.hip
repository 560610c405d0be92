/*
 * ccl_api.hip -- C-ABI of the connected components and the island removal (include/sift3d.h, "connected components of a label
 * volume"): sift3d_label_components and sift3d_clean_labels.  The kernels are in kernels_ccl.hip; the defaults,
 * the checks of the extents and the parameters and the report's text are host code (ccl_host.c), the label check the fusion's
 * (fuse_host.c).
 */
#include <cmath>
#include <cstring>
#include <vector>

#include "device_call.h"

hipError_t sift3d_launch_ccl_bricks(hipStream_t s, int conn, const unsigned short *lab, const unsigned long long *valid, int64_t nx, int64_t ny, int64_t nz,
                                    unsigned *parent);
hipError_t sift3d_launch_ccl_merge(hipStream_t s, int conn, const unsigned short *lab, const unsigned long long *valid, int64_t nx, int64_t ny, int64_t nz,
                                   unsigned *parent);
hipError_t sift3d_launch_ccl_flatten(hipStream_t s, const unsigned *parent, int64_t n, unsigned *root, int *flag);
hipError_t sift3d_launch_ccl_number(hipStream_t s, unsigned *root, const int *num, const int *flag, const unsigned short *lab, int64_t nx, int64_t ny, int64_t n,
                                    sift3d_component_record *rec);
hipError_t sift3d_launch_ccl_records(hipStream_t s, const unsigned *comp, int64_t nx, int64_t ny, int64_t n, sift3d_component_record *rec);
hipError_t sift3d_launch_ccl_sizes(hipStream_t s, const unsigned *comp, int64_t nx, int64_t n, unsigned *size);
hipError_t sift3d_launch_ccl_small(hipStream_t s, const unsigned *size, int64_t ncomp, unsigned min_voxels, int *small);
hipError_t sift3d_launch_ccl_votes(hipStream_t s, const unsigned *comp, const unsigned short *lab, const int *small, const int *sidx, const unsigned short *lidx,
                                   int64_t nx, int64_t ny, int64_t nz, int nl, unsigned *votes);
hipError_t sift3d_launch_ccl_decide(hipStream_t s, const int *small, const int *sidx, const unsigned *size, const unsigned *votes, const unsigned short *present,
                                    int nl, int64_t ncomp, unsigned *fresh, unsigned long long *counts);
hipError_t sift3d_launch_ccl_apply(hipStream_t s, const unsigned *comp, const int *small, const int *sidx, const unsigned *fresh, int64_t n, float *labels);

#define CCL_EVENTS SIFT3D_CCL_STAGES /* one before the label plane and one after each of the five steps */

/* the planes of one labelling and the events around its steps */
struct ccl_planes {
    float *f = nullptr;                 /* the labels */
    unsigned short *lab = nullptr;      /* uint16 plane */
    unsigned long long *valid = nullptr; /* a bit per voxel */
    unsigned *parent = nullptr;         /* the parent plane; after the flatten the scan's output */
    unsigned *root = nullptr;           /* the roots; after the numbering the component map */
    int *flag = nullptr;                /* the root flags; in the cleaning then the small flags */
    void *scan_tmp = nullptr;
    size_t scan_bytes = 0;
    stage_events<CCL_EVENTS> ev;
    /* false without memory */
    bool alloc(device_call &dc, size_t nv)
    {
        scan_bytes = sift3d_scan_temp_bytes((int64_t)nv) + 256;
        unsigned char *tmp = nullptr;
        const bool ok = dc.alloc(&f, nv) == hipSuccess && dc.alloc(&lab, nv) == hipSuccess && dc.alloc(&valid, (nv + 63) / 64) == hipSuccess &&
                        dc.alloc(&parent, nv) == hipSuccess && dc.alloc(&root, nv) == hipSuccess && dc.alloc(&flag, nv) == hipSuccess &&
                        dc.alloc(&tmp, scan_bytes) == hipSuccess;
        scan_tmp = tmp;
        return ok;
    }
    /* the first half: f to the roots, their flags and the flags' scan (in the parent plane); *ncomp the number of components.
     * Synchronises, since the caller sizes the records by the count. */
    hipError_t label(device_call &dc, int conn, int64_t nx, int64_t ny, int64_t nz, int64_t *ncomp)
    {
        const int64_t n = nx * ny * nz;
        int last[2] = {0, 0};
        hipError_t rc = ev.record(0, dc.s);
        if (rc == hipSuccess) rc = sift3d_launch_label_plane(dc.s, f, n, lab, valid);
        if (rc == hipSuccess) rc = ev.record(1, dc.s);
        if (rc == hipSuccess) rc = sift3d_launch_ccl_bricks(dc.s, conn, lab, valid, nx, ny, nz, parent);
        if (rc == hipSuccess) rc = ev.record(2, dc.s);
        if (rc == hipSuccess) rc = sift3d_launch_ccl_merge(dc.s, conn, lab, valid, nx, ny, nz, parent);
        if (rc == hipSuccess) rc = ev.record(3, dc.s);
        if (rc == hipSuccess) rc = sift3d_launch_ccl_flatten(dc.s, parent, n, root, flag);
        if (rc == hipSuccess) rc = ev.record(4, dc.s);
        /* the parent plane is free: it takes the scan */
        if (rc == hipSuccess) rc = sift3d_scan_counts(dc.s, scan_tmp, scan_bytes, flag, (int *)parent, n);
        if (rc == hipSuccess) rc = dc.download(&last[0], (const int *)parent + (n - 1), 1);
        if (rc == hipSuccess) rc = dc.download(&last[1], (const int *)flag + (n - 1), 1);
        if (rc == hipSuccess) rc = dc.sync();
        *ncomp = (int64_t)last[0] + last[1];
        return rc;
    }
    /* the second half: the numbers, and the records where rec is given (device memory for *ncomp of them) */
    hipError_t number(device_call &dc, int64_t nx, int64_t ny, int64_t nz, sift3d_component_record *rec)
    {
        const int64_t n = nx * ny * nz;
        hipError_t rc = sift3d_launch_ccl_number(dc.s, root, (const int *)parent, flag, lab, nx, ny, n, rec);
        if (rc == hipSuccess && rec) rc = sift3d_launch_ccl_records(dc.s, root, nx, ny, n, rec);
        if (rc == hipSuccess) rc = ev.record(5, dc.s);
        return rc;
    }
    /* total, label plane, brick pass, border merge, flatten, numbers and records; the stream has been synchronised */
    hipError_t elapsed(double ms[SIFT3D_CCL_STAGES]) const
    {
        hipError_t rc = ev.elapsed(0, 5, &ms[0]);
        for (int i = 1; i < SIFT3D_CCL_STAGES && rc == hipSuccess; i++) rc = ev.elapsed(i - 1, i, &ms[i]);
        return rc;
    }
};

extern "C" int sift3d_label_components(int device, const float *labels, int64_t nx, int64_t ny, int64_t nz, int32_t connectivity, uint32_t *comp,
                                       sift3d_component_record *records, int64_t max_records, int64_t *n_components, double *kernel_ms, char *err,
                                       int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms)
        for (int i = 0; i < SIFT3D_CCL_STAGES; i++) kernel_ms[i] = 0.0;
    if (n_components) *n_components = 0;
    if (!labels || !n_components) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    if (sift3d_ccl_check_extents(nx, ny, nz, err, err_len) != 0) return SIFT3D_ERR_ARG;
    if (connectivity != 6 && connectivity != 26) return call_fail(err, err_len, SIFT3D_ERR_ARG, "connectivity = %d: 6 or 26", (int)connectivity);
    if (records && max_records < 0) return call_fail(err, err_len, SIFT3D_ERR_ARG, "max_records = %lld: negative", (long long)max_records);
    const int64_t n = nx * ny * nz;
    const int bad = check_labels("", labels, n, err, err_len);
    if (bad != SIFT3D_OK) return bad;

    const size_t nv = (size_t)n;
    device_call dc(err, err_len);
    ccl_planes pl;
    DEVCHK(dc, dc.open(device, false));
    DEVCHK(dc, pl.ev.create());
    if (!pl.alloc(dc, nv)) return dc.no_memory();
    DEVCHK(dc, dc.to_device(pl.f, labels, nv));
    int64_t ncomp = 0;
    DEVCHK(dc, pl.label(dc, connectivity, nx, ny, nz, &ncomp));
    *n_components = ncomp;
    const bool fits = records && ncomp <= max_records;
    sift3d_component_record *d_rec = nullptr;
    if (fits && ncomp > 0 && dc.alloc(&d_rec, (size_t)ncomp) != hipSuccess) return dc.no_memory(" for the records of %lld components", (long long)ncomp);
    DEVCHK(dc, pl.number(dc, nx, ny, nz, d_rec));
    if (comp) DEVCHK(dc, dc.download((unsigned *)comp, pl.root, nv));
    if (d_rec) DEVCHK(dc, dc.download(records, d_rec, (size_t)ncomp));
    DEVCHK(dc, dc.sync());
    if (kernel_ms) DEVCHK(dc, pl.elapsed(kernel_ms));
    if (records && !fits)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "%lld components: more than max_records = %lld (no record written)", (long long)ncomp,
                         (long long)max_records);
    return SIFT3D_OK;
}

extern "C" int sift3d_clean_labels(const float *labels, int64_t nx, int64_t ny, int64_t nz, const sift3d_clean_params *pp, float *out,
                                   sift3d_clean_report *report, double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (report) memset(report, 0, sizeof *report);
    sift3d_clean_params p;
    if (pp) p = *pp;
    else sift3d_clean_defaults(&p);
    if (!labels || !out) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    if (sift3d_ccl_check_extents(nx, ny, nz, err, err_len) != 0) return SIFT3D_ERR_ARG;
    if (sift3d_clean_check(&p, err, err_len) != 0) return SIFT3D_ERR_ARG;
    const int64_t n = nx * ny * nz;
    const int bad = check_labels("", labels, n, err, err_len);
    if (bad != SIFT3D_OK) return bad;
    /* the labels present, in ascending order, and the index of each among them; a round brings no new label */
    std::vector<unsigned short> present, lidx(SIFT3D_LABEL_COUNT, 0);
    {
        std::vector<unsigned char> seen(SIFT3D_LABEL_COUNT, 0);
        for (int64_t i = 0; i < n; i++)
            if (std::isfinite(labels[i])) seen[(int)labels[i]] = 1;
        for (int l = 0; l < SIFT3D_LABEL_COUNT; l++)
            if (seen[l]) {
                lidx[l] = (unsigned short)present.size();
                present.push_back((unsigned short)l);
            }
    }
    const int nl = (int)present.size();

    const size_t nv = (size_t)n;
    device_call dc(err, err_len);
    ccl_planes pl;
    int *d_sidx;
    unsigned short *d_lidx, *d_present;
    unsigned long long *d_counts;
    unsigned *d_votes = nullptr, *d_fresh = nullptr;
    size_t cap_small = 0;
    DEVCHK(dc, dc.open(p.device, false));
    DEVCHK(dc, pl.ev.create());
    if (!pl.alloc(dc, nv) || dc.alloc(&d_sidx, nv) != hipSuccess || dc.alloc(&d_lidx, SIFT3D_LABEL_COUNT) != hipSuccess ||
        dc.alloc(&d_present, SIFT3D_LABEL_COUNT) != hipSuccess || dc.alloc(&d_counts, 4) != hipSuccess)
        return dc.no_memory();
    DEVCHK(dc, dc.to_device(pl.f, labels, nv));
    DEVCHK(dc, dc.to_device(d_lidx, lidx.data(), SIFT3D_LABEL_COUNT));
    if (nl > 0) DEVCHK(dc, dc.to_device(d_present, present.data(), (size_t)nl));
    sift3d_clean_report rep;
    memset(&rep, 0, sizeof rep);
    double total_ms = 0.0;
    for (int r = 0; r < p.rounds; r++) {
        sift3d_clean_round &rr = rep.round[r];
        int64_t ncomp = 0;
        DEVCHK(dc, pl.label(dc, p.connectivity, nx, ny, nz, &ncomp));
        DEVCHK(dc, pl.number(dc, nx, ny, nz, nullptr));
        rep.rounds_run = r + 1;
        rr.components = ncomp;
        int64_t nsmall = 0;
        unsigned *d_size = pl.parent; /* the scan has been used: the plane takes the sizes */
        if (ncomp > 0) {
            int last[2] = {0, 0};
            DEVCHK(dc, hipMemsetAsync(d_size, 0, sizeof(unsigned) * (size_t)ncomp, dc.s));
            DEVCHK(dc, sift3d_launch_ccl_sizes(dc.s, pl.root, nx, n, d_size));
            DEVCHK(dc, sift3d_launch_ccl_small(dc.s, d_size, ncomp, (unsigned)p.min_voxels, pl.flag));
            DEVCHK(dc, sift3d_scan_counts(dc.s, pl.scan_tmp, pl.scan_bytes, pl.flag, d_sidx, ncomp));
            DEVCHK(dc, dc.download(&last[0], (const int *)d_sidx + (ncomp - 1), 1));
            DEVCHK(dc, dc.download(&last[1], (const int *)pl.flag + (ncomp - 1), 1));
            DEVCHK(dc, dc.sync());
            nsmall = (int64_t)last[0] + last[1];
        }
        rr.small = nsmall;
        unsigned long long counts[4] = {0, 0, 0, 0};
        if (nsmall > 0) {
            const int64_t bytes = nsmall * nl * (int64_t)sizeof(unsigned);
            if (bytes > SIFT3D_CLEAN_VOTE_BYTES)
                return call_fail(err, err_len, SIFT3D_ERR_ARG, "round %d: %lld small components and %d labels need a vote table of %lld bytes: more than %lld",
                                 r + 1, (long long)nsmall, nl, (long long)bytes, (long long)SIFT3D_CLEAN_VOTE_BYTES);
            if ((size_t)nsmall > cap_small) {
                if (dc.alloc(&d_votes, (size_t)nsmall * nl) != hipSuccess || dc.alloc(&d_fresh, (size_t)nsmall) != hipSuccess)
                    return dc.no_memory(" for the vote table");
                cap_small = (size_t)nsmall;
            }
            DEVCHK(dc, hipMemsetAsync(d_votes, 0, (size_t)bytes, dc.s));
            DEVCHK(dc, hipMemsetAsync(d_counts, 0, sizeof counts, dc.s));
            DEVCHK(dc, sift3d_launch_ccl_votes(dc.s, pl.root, pl.lab, pl.flag, d_sidx, d_lidx, nx, ny, nz, nl, d_votes));
            DEVCHK(dc, sift3d_launch_ccl_decide(dc.s, pl.flag, d_sidx, d_size, d_votes, d_present, nl, ncomp, d_fresh, d_counts));
            DEVCHK(dc, sift3d_launch_ccl_apply(dc.s, pl.root, pl.flag, d_sidx, d_fresh, n, pl.f));
            DEVCHK(dc, pl.ev.record(5, dc.s)); /* the round ends here */
            DEVCHK(dc, dc.download(counts, d_counts, 4));
        }
        DEVCHK(dc, dc.sync());
        double ms = 0.0;
        DEVCHK(dc, pl.ev.elapsed(0, 5, &ms));
        total_ms += ms;
        rr.resolved = (int64_t)counts[0];
        rr.resolved_voxels = (int64_t)counts[1];
        rr.unresolved = (int64_t)counts[2];
        rr.unresolved_voxels = (int64_t)counts[3];
        if (r == 0) rep.total.components = rr.components;
        rep.total.resolved += rr.resolved;
        rep.total.resolved_voxels += rr.resolved_voxels;
        rep.total.small = rr.small;
        rep.total.unresolved = rr.unresolved;
        rep.total.unresolved_voxels = rr.unresolved_voxels;
        if (rr.resolved == 0) break; /* no voxel changed */
    }
    DEVCHK(dc, dc.download(out, pl.f, nv));
    DEVCHK(dc, dc.sync());
    if (report) *report = rep;
    if (kernel_ms) *kernel_ms = total_ms;
    return SIFT3D_OK;
}
