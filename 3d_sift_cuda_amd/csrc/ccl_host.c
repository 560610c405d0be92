/*
 * ccl_host.c -- host side of the connected components and the island removal: the default parameters, the
 * checks of the extents and of the parameters with their texts, and the report as text.  Linked into libsift3d_hip.so (ccl_api.hip
 * uses it) and into libsift3d_host.so (no GPU needed).
 */
#include <stdarg.h>
#include <stdio.h>

#include "sift3d.h"

void sift3d_clean_defaults(sift3d_clean_params *p)
{
    p->min_voxels = 8;
    p->connectivity = 6;
    p->rounds = 4;
    p->device = 0;
}

__attribute__((format(printf, 3, 4))) static int refuse(char *err, int64_t err_len, const char *fmt, ...)
{
    if (err && err_len > 0) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, (size_t)err_len, fmt, ap);
        va_end(ap);
    }
    return -1;
}

int sift3d_ccl_check_extents(int64_t nx, int64_t ny, int64_t nz, char *err, int64_t err_len)
{
    const int64_t ext[3] = {nx, ny, nz};
    const char *axis[3] = {"nx", "ny", "nz"};
    for (int c = 0; c < 3; c++)
        if (ext[c] < 1 || ext[c] > SIFT3D_CCL_MAX_EXTENT)
            return refuse(err, err_len, "%s = %lld: an extent must be 1 .. %d", axis[c], (long long)ext[c], SIFT3D_CCL_MAX_EXTENT);
    if (nx * ny * nz > SIFT3D_CCL_MAX_VOXELS) return refuse(err, err_len, "nx ny nz = %lld: more than 2^30 voxels", (long long)(nx * ny * nz));
    return 0;
}

int sift3d_clean_check(const sift3d_clean_params *p, char *err, int64_t err_len)
{
    if (!p) return refuse(err, err_len, "null pointer");
    if (p->min_voxels < 1 || p->min_voxels > SIFT3D_CLEAN_MAX_MIN_VOXELS)
        return refuse(err, err_len, "min_voxels = %d: 1 .. %d", (int)p->min_voxels, SIFT3D_CLEAN_MAX_MIN_VOXELS);
    if (p->connectivity != 6 && p->connectivity != 26) return refuse(err, err_len, "connectivity = %d: 6 or 26", (int)p->connectivity);
    if (p->rounds < 1 || p->rounds > SIFT3D_CLEAN_MAX_ROUNDS) return refuse(err, err_len, "rounds = %d: 1 .. %d", (int)p->rounds, SIFT3D_CLEAN_MAX_ROUNDS);
    return 0;
}

/* appends to buf[at ..) what fits, returns the position the whole text has reached */
__attribute__((format(printf, 4, 5))) static int64_t put(char *buf, int64_t len, int64_t at, const char *fmt, ...)
{
    char line[256];
    va_list ap;
    va_start(ap, fmt);
    const int n = vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    for (int i = 0; i < n; i++)
        if (buf && at + i < len - 1) buf[at + i] = line[i];
    return at + n;
}

static int64_t put_round(char *buf, int64_t len, int64_t at, const char *head, const sift3d_clean_round *r)
{
    return put(buf, len, at, "%s\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\n", head, (long long)r->components, (long long)r->small, (long long)r->resolved,
               (long long)r->resolved_voxels, (long long)r->unresolved, (long long)r->unresolved_voxels);
}

int64_t sift3d_clean_report_text(const sift3d_clean_report *rep, char *buf, int64_t len)
{
    if (!rep) return -1;
    int64_t at = put(buf, len, 0, "# round components small resolved resolved_voxels unresolved unresolved_voxels\n");
    const int rounds = rep->rounds_run < 0 ? 0 : rep->rounds_run > SIFT3D_CLEAN_MAX_ROUNDS ? SIFT3D_CLEAN_MAX_ROUNDS : rep->rounds_run;
    for (int r = 0; r < rounds; r++) {
        char head[16];
        snprintf(head, sizeof head, "%d", r + 1);
        at = put_round(buf, len, at, head, &rep->round[r]);
    }
    at = put_round(buf, len, at, "# total", &rep->total);
    at = put(buf, len, at, "# rounds run %d\n", rounds);
    if (buf && len > 0) buf[at < len - 1 ? at : len - 1] = 0;
    return at;
}
