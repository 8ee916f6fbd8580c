// index_merge.hip -- K4m `csr_merge`: the live index's delta segment folded into main without a sort (DESIGN 4b "Live
// ingest"; plan and work split: aidfp_live_plan.h). Both CSRs share the key space and the bucket order and the delta's
// postings arrived later, so the folded CSR is off_new[k] = off_main[k] + off_delta[k], each bucket main's run followed
// by the delta's, signatures alongside: one streaming pass of about 2 x 10 B per posting, where the radix build moves
// 80 B and needs 16 B per posting of scratch. Three launches: the new offsets (element-wise), the tiles' posting
// totals (the host cuts them into work items), and the merge proper over the items.
#include "aidfp_device.h"
#include "aidfp_launch.h"
#include "aidfp_live_plan.h"

namespace aid {

// off_new = off_main + off_delta over n entries; n4 groups of four through 16-B accesses, the tail one by one
__global__ __launch_bounds__(256) void k_merge_offsets(const uint32_t *__restrict__ om, const uint32_t *__restrict__ od,
                                                       uint32_t *__restrict__ on, int64_t n) {
    const int64_t n4 = n / 4, stride = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint4 *m4 = reinterpret_cast<const uint4 *>(om), *d4 = reinterpret_cast<const uint4 *>(od);
    uint4 *o4 = reinterpret_cast<uint4 *>(on);
    for (int64_t i = tid; i < n4; i += stride) {
        const uint4 a = m4[i], b = d4[i];
        o4[i] = make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    for (int64_t i = 4 * n4 + tid; i < n; i += stride) on[i] = om[i] + od[i];
}

// destination postings of every tile of kMergeTileKeys keys
__global__ __launch_bounds__(256) void k_merge_tile_totals(const uint32_t *__restrict__ om, const uint32_t *__restrict__ od,
                                                           uint32_t *__restrict__ total, int n_tiles) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    const size_t k0 = (size_t)t * kMergeTileKeys, k1 = k0 + kMergeTileKeys;
    total[t] = (om[k1] - om[k0]) + (od[k1] - od[k0]);
}

// One work item per workgroup: destination postings [first, first + count) of its tile. The tile's offsets of both
// segments sit in LDS; the bucket of a destination posting is found there by bisection over the merged local offsets
// L(i) = (om[i] - om[0]) + (od[i] - od[0]) (the largest i with L(i) <= j: empty buckets are skipped by construction),
// and its source follows: position r = j - L(i) of the bucket is main's r-th posting while r < main's run length, else
// the delta's. A lane takes the two postings of an even absolute destination index, so that inside an item every
// store is one aligned 16-B access (and 4 B of signatures); an item's odd first or last posting is stored alone.
__device__ __forceinline__ int merge_bucket(const uint32_t *s_m, const uint32_t *s_d, uint32_t j) {
    const uint32_t bm = s_m[0], bd = s_d[0];
    int lo = 0, hi = kMergeTileKeys;  // L(lo) <= j < L(hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((s_m[mid] - bm) + (s_d[mid] - bd) <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_csr_merge(const MergeItem *__restrict__ items, const uint32_t *__restrict__ om,
                                                   const uint64_t *__restrict__ pm, const uint16_t *__restrict__ sm,
                                                   const uint32_t *__restrict__ od, const uint64_t *__restrict__ pd,
                                                   const uint16_t *__restrict__ sd, uint64_t *__restrict__ pn,
                                                   uint16_t *__restrict__ sn) {
    __shared__ uint32_t s_m[kMergeTileKeys + 1], s_d[kMergeTileKeys + 1];
    const MergeItem it = items[blockIdx.x];
    const size_t k0 = (size_t)it.tile * kMergeTileKeys;
    for (int i = threadIdx.x; i <= kMergeTileKeys; i += 256) {
        s_m[i] = om[k0 + i];
        s_d[i] = od[k0 + i];
    }
    __syncthreads();
    const uint32_t bm = s_m[0], bd = s_d[0];
    const uint64_t dst0 = (uint64_t)bm + bd;  // the tile's first destination posting
    const uint64_t a0 = dst0 + it.first, a1 = a0 + it.count;
    for (uint64_t p = (a0 & ~(uint64_t)1) + 2 * (uint64_t)threadIdx.x; p < a1; p += 512) {
        uint64_t post[2] = {0, 0};
        uint16_t sig[2] = {0, 0};
        bool have[2];
        int b = -1;
        for (int e = 0; e < 2; ++e) {
            const uint64_t a = p + e;
            have[e] = a >= a0 && a < a1;
            if (!have[e]) continue;
            const uint32_t j = (uint32_t)(a - dst0);
            if (b < 0 || (s_m[b + 1] - bm) + (s_d[b + 1] - bd) <= j) b = merge_bucket(s_m, s_d, j);
            const uint32_t r = j - ((s_m[b] - bm) + (s_d[b] - bd)), run = s_m[b + 1] - s_m[b];
            if (r < run) {
                post[e] = pm[(size_t)s_m[b] + r];
                sig[e] = sm[(size_t)s_m[b] + r];
            } else {
                post[e] = pd[(size_t)s_d[b] + (r - run)];
                sig[e] = sd[(size_t)s_d[b] + (r - run)];
            }
        }
        if (have[0] && have[1]) {
            *reinterpret_cast<ulonglong2 *>(pn + p) = make_ulonglong2(post[0], post[1]);
            *reinterpret_cast<uint32_t *>(sn + p) = (uint32_t)sig[0] | ((uint32_t)sig[1] << 16);
        } else if (have[0]) {
            pn[p] = post[0];
            sn[p] = sig[0];
        } else if (have[1]) {
            pn[p + 1] = post[1];
            sn[p + 1] = sig[1];
        }
    }
}

void launch_csr_merge_offsets(const uint32_t *om, const uint32_t *od, uint32_t *on, int64_t n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_merge_offsets, dim3(2048), dim3(256), 0, s, om, od, on, n);
}

void launch_csr_merge_totals(const uint32_t *om, const uint32_t *od, uint32_t *total, int n_tiles, hipStream_t s) {
    if (n_tiles > 0)
        hipLaunchKernelGGL(k_merge_tile_totals, dim3((unsigned)((n_tiles + 255) / 256)), dim3(256), 0, s, om, od, total,
                           n_tiles);
}

void launch_csr_merge(const void *items, int64_t n_items, const uint32_t *om, const uint64_t *pm, const uint16_t *sm,
                      const uint32_t *od, const uint64_t *pd, const uint16_t *sd, uint64_t *pn, uint16_t *sn,
                      hipStream_t s) {
    if (n_items > 0)
        hipLaunchKernelGGL(k_csr_merge, dim3((unsigned)n_items), dim3(256), 0, s, static_cast<const MergeItem *>(items), om,
                           pm, sm, od, pd, sd, pn, sn);
}

}  // namespace aid
