/*
 * guided_accept.h -- the accept rule of the guided re-matching, shared by the similarity loop
 * (refine_api.hip) and the field (field_api.hip).  Internal: nothing here is part of the C-ABI.
 */
#ifndef SIFT3D_GUIDED_ACCEPT_H
#define SIFT3D_GUIDED_ACCEPT_H
#include <algorithm>
#include <cstdint>
#include <vector>

/* Accept moving record m when i1[m] >= 0 and (i2[m] < 0 or ratio_num * d2 > ratio_den * d1 in int64); where several accepted
 * records claim one fixed record, the least (d1, moving index) keeps it.  best: n_fixed entries of scratch.  The pairs come
 * back by moving index: pm (moving), pf (fixed), pd (d1). */
static inline void guided_accept(size_t n_moving, const int32_t *i1, const int32_t *d1, const int32_t *i2, const int32_t *d2, int32_t ratio_num,
                                 int32_t ratio_den, std::vector<int32_t> &best, std::vector<int32_t> &pm, std::vector<int32_t> &pf,
                                 std::vector<int32_t> &pd)
{
    const size_t M = n_moving;
    std::fill(best.begin(), best.end(), -1);
    std::vector<char> acc(M, 0);
    for (size_t m = 0; m < M; m++) {
        if (i1[m] < 0) continue;
        if (!(i2[m] < 0 || (int64_t)ratio_num * d2[m] > (int64_t)ratio_den * d1[m])) continue;
        acc[m] = 1;
        int32_t &b = best[i1[m]];
        if (b < 0 || d1[m] < d1[b]) b = (int32_t)m; /* m ascending: a tie keeps the lower index */
    }
    pm.clear();
    pf.clear();
    pd.clear();
    for (size_t m = 0; m < M; m++)
        if (acc[m] && best[i1[m]] == (int32_t)m) {
            pm.push_back((int32_t)m);
            pf.push_back(i1[m]);
            pd.push_back(d1[m]);
        }
}

#endif
