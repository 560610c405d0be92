/*
 * ccl_oracle.c -- CPU oracle of the connected components and the island removal (include/sift3d.h,
 * "connected components of a label volume").  Test infrastructure: built by tests/_helpers.c_oracle, never linked into the product.
 *
 * The components are a flood fill with an explicit queue, started at every voxel in index order that no fill has reached: the
 * first voxel of a fill is the component's key, and the numbers come out in key order by themselves.  There are no bricks, no
 * union-find and no scans, so it shares no structure with the kernels.  The records are taken while filling; the rounds are written
 * out serially as the contract states them.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    int32_t label, reserved;
    int64_t voxels, first;
    int32_t box[6];
} occ_record;

typedef struct {
    int64_t components, small, resolved, resolved_voxels, unresolved, unresolved_voxels;
} occ_round;

typedef struct {
    int32_t rounds_run, reserved;
    occ_round round[16];
    occ_round total;
} occ_report;

/* comp: one uint32 per voxel.  rec (may be NULL): room for max_rec records; those beyond are not written.  Returns the number of
 * components, or -1 without memory or for a connectivity that is none. */
int64_t occ_label(const float *lab, int64_t nx, int64_t ny, int64_t nz, int conn, uint32_t *comp, occ_record *rec, int64_t max_rec)
{
    const int64_t n = nx * ny * nz;
    if (conn != 6 && conn != 26) return -1;
    int64_t *queue = (int64_t *)malloc(sizeof(int64_t) * (size_t)n);
    if (!queue) return -1;
    memset(comp, 0, sizeof(uint32_t) * (size_t)n);
    int64_t count = 0;
    for (int64_t start = 0; start < n; start++) {
        if (comp[start] != 0 || !isfinite(lab[start])) continue;
        const float l = lab[start];
        occ_record r = {(int32_t)l, 0, 0, start, {INT32_MAX, -1, INT32_MAX, -1, INT32_MAX, -1}};
        count++;
        int64_t head = 0, tail = 0;
        queue[tail++] = start;
        comp[start] = (uint32_t)count;
        while (head < tail) {
            const int64_t i = queue[head++];
            const int64_t x = i % nx, y = i / nx % ny, z = i / (nx * ny);
            r.voxels++;
            if (x < r.box[0]) r.box[0] = (int32_t)x;
            if (x > r.box[1]) r.box[1] = (int32_t)x;
            if (y < r.box[2]) r.box[2] = (int32_t)y;
            if (y > r.box[3]) r.box[3] = (int32_t)y;
            if (z < r.box[4]) r.box[4] = (int32_t)z;
            if (z > r.box[5]) r.box[5] = (int32_t)z;
            for (int dz = -1; dz <= 1; dz++)
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int steps = (dx != 0) + (dy != 0) + (dz != 0);
                        if (steps == 0 || (conn == 6 && steps != 1)) continue;
                        const int64_t ax = x + dx, ay = y + dy, az = z + dz;
                        if (ax < 0 || ax >= nx || ay < 0 || ay >= ny || az < 0 || az >= nz) continue;
                        const int64_t j = (az * ny + ay) * nx + ax;
                        if (comp[j] != 0 || !isfinite(lab[j]) || lab[j] != l) continue;
                        comp[j] = (uint32_t)count;
                        queue[tail++] = j;
                    }
        }
        if (rec && count <= max_rec) rec[count - 1] = r;
    }
    free(queue);
    return count;
}

/* one round: in to out; 0, or -1 without memory */
static int one_round(const float *in, int64_t nx, int64_t ny, int64_t nz, int64_t min_voxels, int conn, float *out, occ_round *rr)
{
    const int64_t n = nx * ny * nz;
    uint32_t *comp = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)n);
    int64_t *votes = (int64_t *)calloc(65536, sizeof(int64_t));
    int32_t *touched = (int32_t *)malloc(sizeof(int32_t) * 65536); /* the labels with a vote: only they are looked at and zeroed again */
    int64_t *size = NULL, *start = NULL, *list = NULL;
    int rc = -1;
    memset(rr, 0, sizeof *rr);
    memcpy(out, in, sizeof(float) * (size_t)n);
    if (!comp || !votes || !touched) goto done;
    const int64_t count = occ_label(in, nx, ny, nz, conn, comp, NULL, 0);
    if (count < 0) goto done;
    rr->components = count;
    size = (int64_t *)calloc((size_t)count + 1, sizeof(int64_t));
    start = (int64_t *)calloc((size_t)count + 2, sizeof(int64_t));
    list = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1));
    if (!size || !start || !list) goto done;
    for (int64_t i = 0; i < n; i++)
        if (comp[i]) size[comp[i] - 1]++;
    /* the voxels of every component, one after the other */
    for (int64_t k = 0; k < count; k++) start[k + 1] = start[k] + size[k];
    {
        int64_t *fill = (int64_t *)malloc(sizeof(int64_t) * ((size_t)count + 1));
        if (!fill) goto done;
        memcpy(fill, start, sizeof(int64_t) * ((size_t)count + 1));
        for (int64_t i = 0; i < n; i++)
            if (comp[i]) list[fill[comp[i] - 1]++] = i;
        free(fill);
    }
    for (int64_t k = 0; k < count; k++) {
        if (size[k] >= min_voxels) continue;
        rr->small++;
        int32_t ntouched = 0;
        for (int64_t v = start[k]; v < start[k + 1]; v++) {
            const int64_t i = list[v], x = i % nx, y = i / nx % ny, z = i / (nx * ny);
            const int64_t face[6][3] = {{x - 1, y, z}, {x + 1, y, z}, {x, y - 1, z}, {x, y + 1, z}, {x, y, z - 1}, {x, y, z + 1}};
            for (int f = 0; f < 6; f++) {
                if (face[f][0] < 0 || face[f][0] >= nx || face[f][1] < 0 || face[f][1] >= ny || face[f][2] < 0 || face[f][2] >= nz) continue;
                const int64_t j = (face[f][2] * ny + face[f][1]) * nx + face[f][0];
                if (comp[j] == 0 || size[comp[j] - 1] < min_voxels) continue; /* unlabelled, or in a small component */
                if (votes[(int32_t)in[j]]++ == 0) touched[ntouched++] = (int32_t)in[j];
            }
        }
        int64_t best = 0;
        int32_t winner = -1;
        for (int32_t c = 0; c < ntouched; c++) {
            const int32_t l = touched[c];
            if (votes[l] > best || (votes[l] == best && l < winner)) { /* the most votes; ties go to the smaller label */
                best = votes[l];
                winner = l;
            }
            votes[l] = 0;
        }
        if (winner < 0) {
            rr->unresolved++;
            rr->unresolved_voxels += size[k];
            continue;
        }
        rr->resolved++;
        rr->resolved_voxels += size[k];
        for (int64_t v = start[k]; v < start[k + 1]; v++) out[list[v]] = (float)winner;
    }
    rc = 0;
done:
    free(comp);
    free(votes);
    free(touched);
    free(size);
    free(start);
    free(list);
    return rc;
}

/* the rounds: in to out (two different arrays); 0, or -1 without memory or for parameters that are none */
int occ_clean(const float *in, int64_t nx, int64_t ny, int64_t nz, int32_t min_voxels, int32_t conn, int32_t rounds, float *out, occ_report *rep)
{
    const int64_t n = nx * ny * nz;
    if (min_voxels < 1 || min_voxels > (1 << 24) || rounds < 1 || rounds > 16 || (conn != 6 && conn != 26)) return -1;
    float *cur = (float *)malloc(sizeof(float) * (size_t)n);
    if (!cur) return -1;
    memcpy(cur, in, sizeof(float) * (size_t)n);
    memset(rep, 0, sizeof *rep);
    int rc = 0;
    for (int r = 0; r < rounds && rc == 0; r++) {
        occ_round *rr = &rep->round[r];
        rc = one_round(cur, nx, ny, nz, min_voxels, conn, out, rr);
        if (rc != 0) break;
        memcpy(cur, out, sizeof(float) * (size_t)n);
        rep->rounds_run = r + 1;
        if (r == 0) rep->total.components = rr->components;
        rep->total.resolved += rr->resolved;
        rep->total.resolved_voxels += rr->resolved_voxels;
        rep->total.small = rr->small;
        rep->total.unresolved = rr->unresolved;
        rep->total.unresolved_voxels = rr->unresolved_voxels;
        if (rr->resolved == 0) break;
    }
    memcpy(out, cur, sizeof(float) * (size_t)n);
    free(cur);
    return rc;
}
