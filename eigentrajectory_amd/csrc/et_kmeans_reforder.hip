// et_kmeans_reforder.hip -- BatchKMeans (EigenTrajectory/kmeans.py) in the REFERENCE's own fp32 summation orders.
//
// The default k-means of this library (et_kmeans.hip) sums the per-cluster coordinates exactly (64-bit fixed point):
// that is what makes its result independent of the launch geometry and of the number of GPUs, but the reference sums
// fp32 in ATen's reduction order, and Lloyd iterations amplify the ~1e-7 difference: over 96 whole runs of the imported
// reference (tests/golden/g7c_batchkmeans_seeds.npz) the exact-sum fit ends with the reference's labels in 32/32 cases
// at N = 1e3, 31/32 at 1e4, 13/32 at 1e5.  This file is the opt-in single-GPU mode that reproduces the reference's
// arithmetic step for step (`BatchKMeans(..., sums="reference-order")`):
//
//   * kmeans.py:180-182  `(data.unsqueeze(-1) * mask.unsqueeze(-3)).sum(dim=-2)`: every (coordinate, cluster) column is
//     ATen's CASCADE sum of its N terms (SumKernel.cpp; restated in oracle/et_oracle.c: eto_kmeans_reforder_sums):
//     4 interleaved lanes (n mod 4), per lane a 4-level cascade with level_step L = 2^max(4, ceil_log2(N/4)/4).
//     Here: reforder_group_kernel -- one work item per (level-1 group of L*L lane terms, lane, column) runs the two
//     inner levels sequentially; reforder_finish_kernel -- one work item per (lane, column) runs the two outer levels,
//     then per column the N mod 4 leftover terms and the lane combination.  Non-members contribute x*0 = +-0, which
//     leaves a running sum that started at +0 unchanged, so only members are added.
//   * kmeans.py:73-74    `a.pow(2).sum(dim=-2)`: the same kernel's OUTER reduction over the d rows; which of its two
//     orders a column gets depends on its position (blocks of 32 columns: rows in sequence; the columns after the last
//     full block: rows dealt onto 4 lanes -> ((((s0+s4)+s5)+s1)+s2)+s3 for d = 6; fewer than 8 columns: blocks of 4).
//   * kmeans.py:45-51    `diff.sum()`: the kernel's INNER (contiguous) reduction over the d K squared differences.
//   * kmeans.py:88-112   the farthest-first seeding re-evaluates euc_sim against ALL current centroids at every step, and
//     the order of a centroid's norm depends on how many centroids there are: reproduced literally.
//   * a^T b is a fused multiply-add chain from 0 (MKL sgemm with k = 6 on the reference's host; verified bit for bit).
//
// Everything here is plain and serial where the reference's order is serial; it is NOT the fast path (N = 1e5, K = 20:
// ~0.1 ms per iteration against 12 us) and it does not shard: the order of the sums is a property of the whole array.
// Third-party arithmetic (torch 2.10.0 CPU, AVX2-width Vectorized<float>) pinned by tests/test_oracle_golden.py
// (oracle == torch on random inputs) and tests/golden/g7c_* (whole runs of the imported reference).
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "et_common.h"
#include "et_hostring.h"
#include "et_mfma_filter.h"
#include "et_options.h"

#include "et_reforder_plain.inl"
#include "et_reforder_fast_geometry.inl"
#include "et_reforder_fast_assign.inl"
#include "et_reforder_fast_update.inl"
#include "et_reforder_sharded.inl"
#include "et_reforder_host.inl"
