// The shadow check's comparison (include/gzero_nn.h gz_shadow_stats): two sets of head outputs of
// the same rows -- "a", the net's, wherever its segments put them (HBM or pinned host memory), and
// "b", the shadow's, contiguous in HBM -- compared on the device by two kernels.
//
//   shadow_row_kernel   one wave per row: |a - b|, KL(b || a), the first-maximum indices and a
//                       finiteness flag over the row's policies and values, element math in double,
//                       reduced into one RowRecord
//   shadow_fold_kernel  one workgroup: a check's records, in row order, into the cumulative block
//
// Every sum has one fixed order, so the same checks give the same bits: within a role each lane adds
// its elements (lane, lane + 64, ...) in ascending order, the 64 lane sums meet in an xor butterfly
// (offsets 32, 16, 8, 4, 2, 1), a row adds its roles in role order and the fold adds the rows in
// row order.  tests/test_nn_shadow_gpu.py restates exactly this in numpy.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/gzero_nn.h"

namespace gzshadow {

constexpr int kMaxSegments = GZ_MAX_SEGMENTS;
constexpr int kRowsPerBlock = 4;   // waves (rows) per shadow_row_kernel workgroup

struct SegmentA {                  // one run of the net's rows
    int row0;                      // first row of the run within the check
    const float* pol[GZ_MAX_ROLES];
    const float* val;
};

struct RowRecord {
    double max_dp, sum_dp;         // over the row's policy elements, roles in order
    double max_kl, sum_kl;         // over the row's roles (untouched in logits mode)
    double max_dv, sum_dv;
    int argmax_mismatch;           // roles whose first-maximum index differs
    int nonfinite;                 // a non-finite value on either side: the row is left out of the totals
};

struct CompareArgs {
    SegmentA seg[kMaxSegments];    // rows past the last segment's row0 belong to it
    int nseg;
    int n;                         // rows to compare
    int R, V;
    int P[GZ_MAX_ROLES];
    const float* pol_b[GZ_MAX_ROLES];   // [n][P_r]
    const float* val_b;                 // [n][V]
    int logits;                    // the outputs are logits: no KL
    RowRecord* rec;                // [n]
};

// Queues both kernels on `stream`: the rows' records, then their fold into *d_acc (device memory;
// fresh != 0: the block starts from zero).  check_index is what worst_check reports.  Returns NULL,
// or the launch error's text.
const char* launch_compare(const CompareArgs& a, long check_index, int fresh, gz_shadow_stats* d_acc, hipStream_t stream);

}  // namespace gzshadow
