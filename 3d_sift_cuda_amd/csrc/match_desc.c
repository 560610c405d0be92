/*
 * match_desc.c -- the descriptor bytes both matcher paths search (see match.h): linked into libsift3d_host.so and, for the
 * alignment path's records-in entry points (align_api.hip), into libsift3d_hip.so.
 */
#include "match.h"

int sift3d_match_descriptors(const sift3d_feature *f, int64_t n, int8_t *out)
{
    /* The reference hands the floats to FLANN as they are; the rank transform leaves whole numbers 0..63 there.  The search
     * here works on bytes, so anything that is not a whole number in 0..127 is refused -- tested on the float, because a
     * cast of an out-of-range float to char is undefined (advisor, round 3) and would wrap some of them into range. */
    for (int64_t i = 0; i < n; i++)
        for (int j = 0; j < SIFT3D_DESC_LEN; j++) {
            const float d = f[i].desc[j];
            if (!(d >= 0.0f && d <= 127.0f) || d != (float)(int)d) return -1;
            out[i * SIFT3D_DESC_LEN + j] = (int8_t)(int)d;
        }
    return 0;
}
