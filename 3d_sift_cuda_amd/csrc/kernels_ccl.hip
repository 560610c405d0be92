/*
 * kernels_ccl.hip -- connected components of a label volume and the island removal for gfx950 (MI355X; DESIGN.md section 7m;
 * tests/ccl_oracle.c restates them as a serial flood fill).  Everything is integers, minima and counts, so nothing depends on the
 * tiling, the launch order or the order the atomics arrive in.
 *
 * The label plane (uint16 labels and one validity bit per voxel) is kernels_label.hip's label_plane_kernel.
 * ccl_brick_kernel      one workgroup per brick of 32 x 8 x 4 voxels: a union-find in LDS over the brick's voxels.  Every voxel is
 *                       united with its backward neighbours of equal label inside the brick (3 under connectivity 6, 13 under 26)
 *                       by atomicMin on the LDS parent words; the tree is flattened and every voxel writes the global linear index
 *                       of its root to the parent plane (CCL_NONE for an unlabelled voxel).  Local and global indices order the
 *                       voxels of one brick alike, so the smallest local index is the smallest global one.
 * ccl_merge_kernel      a launch of its own: every voxel with a backward neighbour in another brick is united with it in the
 *                       parent plane.  Workgroups on different XCDs read and write the same words here, so every access to the
 *                       plane is a device-scope atomic.
 * ccl_flatten_kernel    a launch of its own, into a second plane: the root of every voxel and the flag "this voxel is a root".
 * ccl_number_kernel     after the exclusive scan of the flags: roots start their records, every voxel turns its root into its
 *                       component's number (in place: a thread reads and writes only its own word of the plane).
 * ccl_record_kernel     voxels and boxes of the records; ccl_size_kernel the voxels alone (the cleaning needs no more).  Both
 *                       aggregate first: a run of voxels of one component along x inside a wave is its first lane's business,
 *                       and a workgroup gathers the runs of its stretch of the volume in 64 LDS slots, which it adds to the
 *                       records once at its end.  A wave whose 64 voxels share a component issues one set of LDS atomics.
 * ccl_small_kernel      the flag "smaller than min_voxels" per component; its scan gives the small components dense indices.
 * ccl_vote_kernel       every voxel of a small component adds one to votes[small index][label index] per face neighbour in a kept
 *                       component.
 * ccl_decide_kernel     one thread per component: a small one takes the label of the most votes (ties: the smaller label) or is
 *                       unresolved; the four counts of the round's report.
 * ccl_apply_kernel      rewrites the voxels of resolved components in place; every other voxel keeps its bits.
 */
#include <algorithm>

#include "sift3d_internal.h"
#include "label_plane.h"

#define CCL_THREADS 256
#define CCL_BX 32
#define CCL_BY 8
#define CCL_BZ 4
#define CCL_BRICK (CCL_BX * CCL_BY * CCL_BZ)
#define CCL_MAX_BLOCKS 2048 /* of every launch here: the kernels go round a grid loop beyond it */
#define CCL_NONE 0xffffffffu

/* the c-th of the 13 backward neighbours (those of a smaller linear index); under connectivity 6 only c = 4, 10 and 12 count */
template <int CONN> __device__ __forceinline__ bool ccl_backward(int c, int &dx, int &dy, int &dz)
{
    if (c < 9) {
        dz = -1;
        dy = c / 3 - 1;
        dx = c % 3 - 1;
    } else if (c < 12) {
        dz = 0;
        dy = -1;
        dx = c - 10;
    } else {
        dz = 0;
        dy = 0;
        dx = -1;
    }
    return CONN == 26 || c == 4 || c == 10 || c == 12;
}

/* A parent word never exceeds its index and only ever decreases, so the walk goes over strictly decreasing indices and ends. */
__device__ __forceinline__ unsigned ccl_lds_find(unsigned *par, unsigned x)
{
    for (;;) {
        const unsigned p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) return x;
        x = p;
    }
}

/* The larger root is hung below the smaller one.  Where another thread got there first (old != a), the word now holds
 * min(old, b), and what remains is to unite old with b: both are smaller than a, so every retry works on smaller indices. */
__device__ __forceinline__ void ccl_lds_unite(unsigned *par, unsigned a, unsigned b)
{
    for (;;) {
        a = ccl_lds_find(par, a);
        b = ccl_lds_find(par, b);
        if (a == b) return;
        if (a < b) {
            const unsigned t = a;
            a = b;
            b = t;
        }
        const unsigned old = atomicMin(&par[a], b);
        if (old == a) return;
        a = old;
    }
}

template <int CONN>
__global__ __launch_bounds__(CCL_THREADS) void ccl_brick_kernel(const unsigned short *__restrict__ lab, const unsigned long long *__restrict__ valid, int nx,
                                                                int ny, int nz, int bxn, int byn, int nbricks, unsigned *__restrict__ parent)
{
    __shared__ unsigned par[CCL_BRICK];
    __shared__ int lb[CCL_BRICK];
    const int lx = threadIdx.x & (CCL_BX - 1), ly = threadIdx.x / CCL_BX;
    for (int b = blockIdx.x; b < nbricks; b += gridDim.x) {
        const int x0 = b % bxn * CCL_BX, y0 = b / bxn % byn * CCL_BY, z0 = b / (bxn * byn) * CCL_BZ;
        const int x = x0 + lx, y = y0 + ly;
        __syncthreads(); /* the brick before is no longer read */
        for (int lz = 0; lz < CCL_BZ; lz++) {
            const int z = z0 + lz, l = (lz * CCL_BY + ly) * CCL_BX + lx;
            int v = -1; /* outside the volume or unlabelled: joined with nothing */
            if (x < nx && y < ny && z < nz) {
                const long long i = ((long long)z * ny + y) * nx + x;
                if (label_valid(valid, i)) v = lab[i];
            }
            lb[l] = v;
            par[l] = (unsigned)l;
        }
        __syncthreads();
        for (int lz = 0; lz < CCL_BZ; lz++) {
            const int l = (lz * CCL_BY + ly) * CCL_BX + lx;
            const int v = lb[l];
            if (v < 0) continue;
            for (int c = 0; c < 13; c++) {
                int dx, dy, dz;
                if (!ccl_backward<CONN>(c, dx, dy, dz)) continue;
                const int ax = lx + dx, ay = ly + dy, az = lz + dz;
                if ((unsigned)ax >= CCL_BX || (unsigned)ay >= CCL_BY || (unsigned)az >= CCL_BZ) continue;
                const int m = (az * CCL_BY + ay) * CCL_BX + ax;
                if (lb[m] == v) ccl_lds_unite(par, (unsigned)l, (unsigned)m);
            }
        }
        __syncthreads();
        for (int lz = 0; lz < CCL_BZ; lz++) {
            const int z = z0 + lz, l = (lz * CCL_BY + ly) * CCL_BX + lx;
            if (x >= nx || y >= ny || z >= nz) continue;
            unsigned out = CCL_NONE;
            if (lb[l] >= 0) {
                const unsigned r = ccl_lds_find(par, (unsigned)l);
                const int rx = x0 + (int)(r % CCL_BX), ry = y0 + (int)(r / CCL_BX % CCL_BY), rz = z0 + (int)(r / (CCL_BX * CCL_BY));
                out = (unsigned)(((long long)rz * ny + ry) * nx + rx);
            }
            parent[((long long)z * ny + y) * nx + x] = out;
        }
    }
}

__device__ __forceinline__ unsigned ccl_load(unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

/* In the merge launch other workgroups, on other XCDs too, change the words this walk reads.  No thread waits for another: a parent
 * word never exceeds its index and only ever decreases (atomicMin is the only write), so the walk goes over strictly decreasing
 * indices and ends whatever it reads.  A load that returns an older value yields an older ancestor, which is still an ancestor. */
__device__ __forceinline__ unsigned ccl_find(unsigned *parent, unsigned x)
{
    for (;;) {
        const unsigned p = ccl_load(&parent[x]);
        if (p == x) return x;
        x = p;
    }
}

/* atomicMin returns the word's true value.  old == a: a was a root and now hangs below b.  Otherwise another thread got there first
 * (or a was no root any more, the find having read an older value): the word now holds min(old, b), and what remains is to unite
 * old with b.  old < a and b < a, so every retry works on strictly smaller indices: the loop ends. */
__device__ __forceinline__ void ccl_unite(unsigned *parent, unsigned a, unsigned b)
{
    for (;;) {
        a = ccl_find(parent, a);
        b = ccl_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const unsigned t = a;
            a = b;
            b = t;
        }
        const unsigned old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

template <int CONN>
__global__ __launch_bounds__(CCL_THREADS) void ccl_merge_kernel(const unsigned short *__restrict__ lab, const unsigned long long *__restrict__ valid, int nx,
                                                                int ny, int nz, long long n, unsigned *parent)
{
    for (long long i = (long long)blockIdx.x * CCL_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CCL_THREADS) {
        const int x = (int)(i % nx), y = (int)(i / nx % ny), z = (int)(i / ((long long)nx * ny));
        const int fx = x % CCL_BX, fy = y % CCL_BY, fz = z % CCL_BZ;
        /* a backward neighbour lies in another brick only from a low face, or, under 26, diagonally across a high x or y face */
        if (!(fx == 0 || fy == 0 || fz == 0 || (CONN == 26 && (fx == CCL_BX - 1 || fy == CCL_BY - 1)))) continue;
        if (!label_valid(valid, i)) continue;
        const unsigned short v = lab[i];
        for (int c = 0; c < 13; c++) {
            int dx, dy, dz;
            if (!ccl_backward<CONN>(c, dx, dy, dz)) continue;
            const int ax = x + dx, ay = y + dy, az = z + dz;
            if (ax < 0 || ax >= nx || ay < 0 || az < 0 || ay >= ny) continue;
            if (ax / CCL_BX == x / CCL_BX && ay / CCL_BY == y / CCL_BY && az / CCL_BZ == z / CCL_BZ) continue; /* the brick pass has done it */
            const long long j = ((long long)az * ny + ay) * nx + ax;
            if (label_valid(valid, j) && lab[j] == v) ccl_unite(parent, (unsigned)i, (unsigned)j);
        }
    }
}

__global__ __launch_bounds__(CCL_THREADS) void ccl_flatten_kernel(const unsigned *__restrict__ parent, long long n, unsigned *__restrict__ root,
                                                                  int *__restrict__ flag)
{
    for (long long i = (long long)blockIdx.x * CCL_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CCL_THREADS) {
        unsigned r = parent[i];
        if (r != CCL_NONE)
            for (unsigned p = parent[r]; p != r; p = parent[r]) r = p; /* nothing writes the plane in this launch */
        root[i] = r;
        flag[i] = r == (unsigned)i ? 1 : 0;
    }
}

/* num: the exclusive scan of flag.  rec (may be NULL): a root starts its component's record.  root becomes the component map. */
__global__ __launch_bounds__(CCL_THREADS) void ccl_number_kernel(unsigned *root, const int *__restrict__ num, const int *__restrict__ flag,
                                                                 const unsigned short *__restrict__ lab, int nx, int ny, long long n,
                                                                 sift3d_component_record *__restrict__ rec)
{
    for (long long i = (long long)blockIdx.x * CCL_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CCL_THREADS) {
        const unsigned r = root[i];
        if (rec && flag[i]) {
            sift3d_component_record &c = rec[num[i]];
            const int x = (int)(i % nx), y = (int)(i / nx % ny), z = (int)(i / ((long long)nx * ny));
            c.label = lab[i];
            c.reserved = 0;
            c.voxels = 0;
            c.first = i;
            c.box[0] = c.box[1] = x;
            c.box[2] = c.box[3] = y;
            c.box[4] = c.box[5] = z;
        }
        root[i] = r == CCL_NONE ? 0u : (unsigned)num[r] + 1u;
    }
}

/* The run of voxels of one component along x that starts at this lane, inside the wave and inside the row: its length, or 0 where
 * the lane starts none or the voxel belongs to no component.  Every lane of the wave calls it. */
__device__ __forceinline__ int ccl_run(int k, int x)
{
    const int lane = threadIdx.x & 63;
    const int before = __shfl_up(k, 1);
    const bool head = lane == 0 || x == 0 || k != before;
    const unsigned long long rest = (__ballot(head) >> lane) >> 1; /* the heads after this lane */
    if (!head || k < 0) return 0;
    return rest ? __ffsll(rest) : 64 - lane;
}

#define CCL_SLOTS 64 /* components a workgroup gathers in LDS at a time */

/* the part of the n voxels that the workgroup takes: a whole number of its 256-voxel steps, one stretch, so that it meets few components */
__device__ __forceinline__ void ccl_stretch(long long n, long long &from, long long &to)
{
    const long long steps = (n + CCL_THREADS - 1) / CCL_THREADS, each = (steps + gridDim.x - 1) / gridDim.x;
    from = min(n, (long long)blockIdx.x * each * CCL_THREADS);
    to = min(n, from + each * CCL_THREADS);
}

/* A workgroup gathers in LDS: the slot k mod 64 belongs to the first component that claims it, a run of that component goes into the
 * slot with LDS atomics, a run of another component that wants the same slot goes to the record directly.  The slots are added to
 * the records once, when the workgroup has seen its stretch: the record of a large component gets a few atomics per workgroup, not a
 * few per wave of voxels, which the chip would queue for. */
__global__ __launch_bounds__(CCL_THREADS) void ccl_record_kernel(const unsigned *__restrict__ comp, int nx, int ny, long long n,
                                                                 sift3d_component_record *rec)
{
    __shared__ int s_k[CCL_SLOTS], s_box[CCL_SLOTS][6];
    __shared__ unsigned s_n[CCL_SLOTS];
    if (threadIdx.x < CCL_SLOTS) {
        s_k[threadIdx.x] = -1;
        s_n[threadIdx.x] = 0;
        for (int c = 0; c < 6; c++) s_box[threadIdx.x][c] = c & 1 ? -1 : 0x7fffffff;
    }
    __syncthreads();
    long long from, to;
    ccl_stretch(n, from, to);
    for (long long base = from; base < to; base += CCL_THREADS) {
        const long long i = base + threadIdx.x;
        const int k = i < n ? (int)comp[i] - 1 : -1;
        const int x = (int)(i % nx), y = (int)(i / nx % ny), z = (int)(i / ((long long)nx * ny));
        const int len = ccl_run(k, x);
        if (len == 0) continue;
        const int slot = k % CCL_SLOTS;
        const int owner = atomicCAS(&s_k[slot], -1, k);
        if (owner == -1 || owner == k) {
            atomicAdd(&s_n[slot], (unsigned)len); /* a stretch has fewer than 2^30 voxels */
            atomicMin(&s_box[slot][0], x);
            atomicMax(&s_box[slot][1], x + len - 1);
            atomicMin(&s_box[slot][2], y);
            atomicMax(&s_box[slot][3], y);
            atomicMin(&s_box[slot][4], z);
            atomicMax(&s_box[slot][5], z);
        } else {
            sift3d_component_record &c = rec[k];
            atomicAdd((unsigned long long *)&c.voxels, (unsigned long long)len);
            atomicMin(&c.box[0], x);
            atomicMax(&c.box[1], x + len - 1);
            atomicMin(&c.box[2], y);
            atomicMax(&c.box[3], y);
            atomicMin(&c.box[4], z);
            atomicMax(&c.box[5], z);
        }
    }
    __syncthreads();
    if (threadIdx.x < CCL_SLOTS && s_k[threadIdx.x] >= 0) {
        sift3d_component_record &c = rec[s_k[threadIdx.x]];
        atomicAdd((unsigned long long *)&c.voxels, (unsigned long long)s_n[threadIdx.x]);
        for (int b = 0; b < 6; b += 2) {
            atomicMin(&c.box[b], s_box[threadIdx.x][b]);
            atomicMax(&c.box[b + 1], s_box[threadIdx.x][b + 1]);
        }
    }
}

/* size: zeroed by the caller; gathered in LDS as in ccl_record_kernel */
__global__ __launch_bounds__(CCL_THREADS) void ccl_size_kernel(const unsigned *__restrict__ comp, int nx, long long n, unsigned *size)
{
    __shared__ int s_k[CCL_SLOTS];
    __shared__ unsigned s_n[CCL_SLOTS];
    if (threadIdx.x < CCL_SLOTS) {
        s_k[threadIdx.x] = -1;
        s_n[threadIdx.x] = 0;
    }
    __syncthreads();
    long long from, to;
    ccl_stretch(n, from, to);
    for (long long base = from; base < to; base += CCL_THREADS) {
        const long long i = base + threadIdx.x;
        const int k = i < n ? (int)comp[i] - 1 : -1;
        const int len = ccl_run(k, (int)(i % nx));
        if (len == 0) continue;
        const int slot = k % CCL_SLOTS;
        const int owner = atomicCAS(&s_k[slot], -1, k);
        if (owner == -1 || owner == k) atomicAdd(&s_n[slot], (unsigned)len);
        else atomicAdd(&size[k], (unsigned)len);
    }
    __syncthreads();
    if (threadIdx.x < CCL_SLOTS && s_k[threadIdx.x] >= 0) atomicAdd(&size[s_k[threadIdx.x]], s_n[threadIdx.x]);
}

__global__ __launch_bounds__(CCL_THREADS) void ccl_small_kernel(const unsigned *__restrict__ size, long long ncomp, unsigned min_voxels, int *__restrict__ small)
{
    for (long long k = (long long)blockIdx.x * CCL_THREADS + threadIdx.x; k < ncomp; k += (long long)gridDim.x * CCL_THREADS)
        small[k] = size[k] < min_voxels ? 1 : 0;
}

/* votes: nsmall rows of nl counts, zeroed by the caller; lidx: the index of a label among those present */
__global__ __launch_bounds__(CCL_THREADS) void ccl_vote_kernel(const unsigned *__restrict__ comp, const unsigned short *__restrict__ lab,
                                                               const int *__restrict__ small, const int *__restrict__ sidx,
                                                               const unsigned short *__restrict__ lidx, int nx, int ny, int nz, long long n, int nl,
                                                               unsigned *votes)
{
    for (long long i = (long long)blockIdx.x * CCL_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CCL_THREADS) {
        const int k = (int)comp[i] - 1;
        if (k < 0 || !small[k]) continue;
        const int x = (int)(i % nx), y = (int)(i / nx % ny), z = (int)(i / ((long long)nx * ny));
        unsigned *row = votes + (size_t)sidx[k] * nl;
        const long long sy = nx, sz = (long long)nx * ny;
        const bool in[6] = {x > 0, x < nx - 1, y > 0, y < ny - 1, z > 0, z < nz - 1};
        const long long at[6] = {i - 1, i + 1, i - sy, i + sy, i - sz, i + sz};
#pragma unroll
        for (int f = 0; f < 6; f++) {
            if (!in[f]) continue;
            const int kj = (int)comp[at[f]] - 1;
            if (kj >= 0 && !small[kj]) atomicAdd(&row[lidx[lab[at[f]]]], 1u);
        }
    }
}

/* present: the nl labels in ascending order.  fresh[s]: the label the small component of index s takes, CCL_NONE for an unresolved
 * one.  counts (zeroed by the caller): resolved components, their voxels, unresolved components, their voxels. */
__global__ __launch_bounds__(CCL_THREADS) void ccl_decide_kernel(const int *__restrict__ small, const int *__restrict__ sidx, const unsigned *__restrict__ size,
                                                                 const unsigned *__restrict__ votes, const unsigned short *__restrict__ present, int nl,
                                                                 long long ncomp, unsigned *__restrict__ fresh, unsigned long long *counts)
{
    for (long long k = (long long)blockIdx.x * CCL_THREADS + threadIdx.x; k < ncomp; k += (long long)gridDim.x * CCL_THREADS) {
        if (!small[k]) continue;
        const int s = sidx[k];
        const unsigned *row = votes + (size_t)s * nl;
        unsigned best = 0;
        int at = -1;
        for (int l = 0; l < nl; l++)
            if (row[l] > best) { /* strictly more: a tie stays with the smaller label */
                best = row[l];
                at = l;
            }
        fresh[s] = at >= 0 ? (unsigned)present[at] : CCL_NONE;
        atomicAdd(&counts[at >= 0 ? 0 : 2], 1ull);
        atomicAdd(&counts[at >= 0 ? 1 : 3], (unsigned long long)size[k]);
    }
}

__global__ __launch_bounds__(CCL_THREADS) void ccl_apply_kernel(const unsigned *__restrict__ comp, const int *__restrict__ small, const int *__restrict__ sidx,
                                                                const unsigned *__restrict__ fresh, long long n, float *__restrict__ labels)
{
    for (long long i = (long long)blockIdx.x * CCL_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CCL_THREADS) {
        const int k = (int)comp[i] - 1;
        if (k < 0 || !small[k]) continue;
        const unsigned l = fresh[sidx[k]];
        if (l != CCL_NONE) labels[i] = (float)l;
    }
}

static unsigned ccl_blocks(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + CCL_THREADS - 1) / CCL_THREADS, CCL_MAX_BLOCKS)); }

/* the callers have checked the extents (1 .. 4096 each, at most 2^30 voxels) and the connectivity (6 or 26) */
hipError_t sift3d_launch_ccl_bricks(hipStream_t s, int conn, const unsigned short *lab, const unsigned long long *valid, int64_t nx, int64_t ny, int64_t nz,
                                    unsigned *parent)
{
    const int bxn = (int)((nx + CCL_BX - 1) / CCL_BX), byn = (int)((ny + CCL_BY - 1) / CCL_BY), bzn = (int)((nz + CCL_BZ - 1) / CCL_BZ);
    const long long nbricks = (long long)bxn * byn * bzn; /* at most 2^30 / 1024 bricks of whole volumes plus the partial ones: below 2^31 */
    if (nbricks > 0x7fffffffll) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<long long>(nbricks, CCL_MAX_BLOCKS);
    if (conn == 26)
        hipLaunchKernelGGL(ccl_brick_kernel<26>, dim3(grid), dim3(CCL_THREADS), 0, s, lab, valid, (int)nx, (int)ny, (int)nz, bxn, byn, (int)nbricks, parent);
    else
        hipLaunchKernelGGL(ccl_brick_kernel<6>, dim3(grid), dim3(CCL_THREADS), 0, s, lab, valid, (int)nx, (int)ny, (int)nz, bxn, byn, (int)nbricks, parent);
    return hipGetLastError();
}

hipError_t sift3d_launch_ccl_merge(hipStream_t s, int conn, const unsigned short *lab, const unsigned long long *valid, int64_t nx, int64_t ny, int64_t nz,
                                   unsigned *parent)
{
    const long long n = nx * ny * nz;
    if (conn == 26)
        hipLaunchKernelGGL(ccl_merge_kernel<26>, dim3(ccl_blocks(n)), dim3(CCL_THREADS), 0, s, lab, valid, (int)nx, (int)ny, (int)nz, n, parent);
    else
        hipLaunchKernelGGL(ccl_merge_kernel<6>, dim3(ccl_blocks(n)), dim3(CCL_THREADS), 0, s, lab, valid, (int)nx, (int)ny, (int)nz, n, parent);
    return hipGetLastError();
}

hipError_t sift3d_launch_ccl_flatten(hipStream_t s, const unsigned *parent, int64_t n, unsigned *root, int *flag)
{
    hipLaunchKernelGGL(ccl_flatten_kernel, dim3(ccl_blocks(n)), dim3(CCL_THREADS), 0, s, parent, (long long)n, root, flag);
    return hipGetLastError();
}

hipError_t sift3d_launch_ccl_number(hipStream_t s, unsigned *root, const int *num, const int *flag, const unsigned short *lab, int64_t nx, int64_t ny, int64_t n,
                                    sift3d_component_record *rec)
{
    hipLaunchKernelGGL(ccl_number_kernel, dim3(ccl_blocks(n)), dim3(CCL_THREADS), 0, s, root, num, flag, lab, (int)nx, (int)ny, (long long)n, rec);
    return hipGetLastError();
}

hipError_t sift3d_launch_ccl_records(hipStream_t s, const unsigned *comp, int64_t nx, int64_t ny, int64_t n, sift3d_component_record *rec)
{
    hipLaunchKernelGGL(ccl_record_kernel, dim3(ccl_blocks(n)), dim3(CCL_THREADS), 0, s, comp, (int)nx, (int)ny, (long long)n, rec);
    return hipGetLastError();
}

hipError_t sift3d_launch_ccl_sizes(hipStream_t s, const unsigned *comp, int64_t nx, int64_t n, unsigned *size)
{
    hipLaunchKernelGGL(ccl_size_kernel, dim3(ccl_blocks(n)), dim3(CCL_THREADS), 0, s, comp, (int)nx, (long long)n, size);
    return hipGetLastError();
}

hipError_t sift3d_launch_ccl_small(hipStream_t s, const unsigned *size, int64_t ncomp, unsigned min_voxels, int *small)
{
    hipLaunchKernelGGL(ccl_small_kernel, dim3(ccl_blocks(ncomp)), dim3(CCL_THREADS), 0, s, size, (long long)ncomp, min_voxels, small);
    return hipGetLastError();
}

hipError_t sift3d_launch_ccl_votes(hipStream_t s, const unsigned *comp, const unsigned short *lab, const int *small, const int *sidx, const unsigned short *lidx,
                                   int64_t nx, int64_t ny, int64_t nz, int nl, unsigned *votes)
{
    const long long n = nx * ny * nz;
    hipLaunchKernelGGL(ccl_vote_kernel, dim3(ccl_blocks(n)), dim3(CCL_THREADS), 0, s, comp, lab, small, sidx, lidx, (int)nx, (int)ny, (int)nz, n, nl, votes);
    return hipGetLastError();
}

hipError_t sift3d_launch_ccl_decide(hipStream_t s, const int *small, const int *sidx, const unsigned *size, const unsigned *votes, const unsigned short *present,
                                    int nl, int64_t ncomp, unsigned *fresh, unsigned long long *counts)
{
    hipLaunchKernelGGL(ccl_decide_kernel, dim3(ccl_blocks(ncomp)), dim3(CCL_THREADS), 0, s, small, sidx, size, votes, present, nl, (long long)ncomp, fresh, counts);
    return hipGetLastError();
}

hipError_t sift3d_launch_ccl_apply(hipStream_t s, const unsigned *comp, const int *small, const int *sidx, const unsigned *fresh, int64_t n, float *labels)
{
    hipLaunchKernelGGL(ccl_apply_kernel, dim3(ccl_blocks(n)), dim3(CCL_THREADS), 0, s, comp, small, sidx, fresh, (long long)n, labels);
    return hipGetLastError();
}
