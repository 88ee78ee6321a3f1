// shadow_compare.h's two kernels.  Plain HIP C++: vector loads and stores, wave shuffles, no atomics
// (one wave owns a row's record, one thread folds the records in order).
#include "shadow_compare.h"

#include <climits>
#include <cmath>

// every double operation rounds as written (the numpy restatement of the tests does the same ones)
#pragma clang fp contract(off)

namespace gzshadow {
namespace {

constexpr double kClip = 1e-30;    // tests/gpu_helpers.kl

// log(x) for a positive, finite, normal x, by the classic reduction x = 2^k (1 + f) with 1 + f in
// [sqrt(2) / 2, sqrt(2)), log(1 + f) = f - f^2 / 2 + s (f^2 / 2 + R(s^2)), s = f / (2 + f), R a degree-7
// minimax polynomial in s^2 (error below 1 ulp).  Only IEEE +, -, *, / in a fixed order, so the numpy
// restatement of the tests gives the same bits: a library log would differ from numpy's by an ulp
// now and then, and the row KLs, sums of terms of both signs, would carry that.
__device__ inline double log_pos(double x) {
    constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    constexpr double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                     Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                     Lg7 = 1.479819860511658591e-01;
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    unsigned hx = (unsigned)(b >> 32);
    hx += 0x3ff00000u - 0x3fe6a09eu;
    const double dk = (double)((int)(hx >> 20) - 0x3ff);
    hx = (hx & 0x000fffffu) + 0x3fe6a09eu;
    const double m = __longlong_as_double((long long)(((unsigned long long)hx << 32) | (b & 0xffffffffull)));
    const double f = m - 1.0;
    const double hf = 0.5 * f;
    const double hfsq = hf * f;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    double t1 = w * Lg6;
    t1 = Lg4 + t1;
    t1 = w * t1;
    t1 = Lg2 + t1;
    t1 = w * t1;
    double t2 = w * Lg7;
    t2 = Lg5 + t2;
    t2 = w * t2;
    t2 = Lg3 + t2;
    t2 = w * t2;
    t2 = Lg1 + t2;
    t2 = z * t2;
    const double R = t2 + t1;
    double r = hfsq + R;
    r = s * r;
    const double klo = dk * ln2_lo;
    r = r + klo;
    r = r - hfsq;
    r = r + f;
    const double khi = dk * ln2_hi;
    r = r + khi;
    return r;
}

__device__ inline double wave_sum(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}
__device__ inline double wave_max(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}
// the first index of the wave's largest value (numpy argmax): lanes hold their own first maximum
__device__ inline int wave_argmax(float v, int i) {
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (ov > v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
    return i;
}

__global__ __launch_bounds__(64 * kRowsPerBlock) void shadow_row_kernel(const CompareArgs A) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= A.n) return;   // (the whole wave)
    int s = 0;
    for (int i = 1; i < A.nseg; ++i)
        if (A.seg[i].row0 <= row) s = i;
    const size_t ra = (size_t)(row - A.seg[s].row0);   // the row within its segment of a
    bool finite = true;
    RowRecord rec{};
    for (int r = 0; r < A.R; ++r) {
        const int P = A.P[r];
        const float* pa = A.seg[s].pol[r] + ra * P;
        const float* pb = A.pol_b[r] + (size_t)row * P;
        double sdp = 0.0, mdp = 0.0, skl = 0.0;
        float besta = -INFINITY, bestb = -INFINITY;
        int ia = INT_MAX, ib = INT_MAX;
        for (int j = lane; j < P; j += 64) {
            const float fa = pa[j], fb = pb[j];
            finite = finite && isfinite(fa) && isfinite(fb);
            const double d = fabs((double)fa - (double)fb);
            sdp = sdp + d;
            mdp = fmax(mdp, d);
            if (!A.logits) {
                const double ref = fmax((double)fb, kClip), got = fmax((double)fa, kClip);
                const double q = ref / got;
                const double t = ref * log_pos(q);
                skl = skl + t;
            }
            if (fa > besta) {
                besta = fa;
                ia = j;
            }
            if (fb > bestb) {
                bestb = fb;
                ib = j;
            }
        }
        sdp = wave_sum(sdp);
        mdp = wave_max(mdp);
        rec.sum_dp = rec.sum_dp + sdp;
        rec.max_dp = fmax(rec.max_dp, mdp);
        if (!A.logits) {
            skl = wave_sum(skl);
            rec.sum_kl = rec.sum_kl + skl;
            rec.max_kl = fmax(rec.max_kl, skl);
        }
        if (wave_argmax(besta, ia) != wave_argmax(bestb, ib)) ++rec.argmax_mismatch;
    }
    const float* va = A.seg[s].val + ra * A.V;
    const float* vb = A.val_b + (size_t)row * A.V;
    for (int v = 0; v < A.V; ++v) {   // (every lane: a handful of values)
        const float fa = va[v], fb = vb[v];
        finite = finite && isfinite(fa) && isfinite(fb);
        const double d = fabs((double)fa - (double)fb);
        rec.sum_dv = rec.sum_dv + d;
        rec.max_dv = fmax(rec.max_dv, d);
    }
    if (!__all(finite ? 1 : 0)) {
        rec = RowRecord{};
        rec.nonfinite = 1;
    }
    if (lane == 0) A.rec[row] = rec;
}

constexpr int kFoldChunk = 256;

__global__ __launch_bounds__(kFoldChunk) void shadow_fold_kernel(const RowRecord* rec, int n, int R, int sumP, int V, int logits,
                                                                 long check_index, int fresh, gz_shadow_stats* acc) {
    __shared__ RowRecord chunk[kFoldChunk];
    gz_shadow_stats t{};
    if (threadIdx.x == 0 && !fresh) t = *acc;
    for (int r0 = 0; r0 < n; r0 += kFoldChunk) {
        const int m = min(kFoldChunk, n - r0);
        __syncthreads();
        if ((int)threadIdx.x < m) chunk[threadIdx.x] = rec[r0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x != 0) continue;
        for (int i = 0; i < m; ++i) {
            const RowRecord& c = chunk[i];
            ++t.rows;
            if (c.nonfinite) {
                ++t.nonfinite_rows;
                continue;
            }
            t.policy_elems += sumP;
            t.value_elems += V;
            if (c.max_dp > t.max_abs_dp) {
                t.max_abs_dp = c.max_dp;
                t.worst_check = check_index;
                t.worst_row = r0 + i;
            }
            t.sum_abs_dp = t.sum_abs_dp + c.sum_dp;
            if (!logits) {
                t.policy_rows += R;
                t.max_row_kl = fmax(t.max_row_kl, c.max_kl);
                t.sum_row_kl = t.sum_row_kl + c.sum_kl;
            }
            t.argmax_mismatch += c.argmax_mismatch;
            t.max_abs_dv = fmax(t.max_abs_dv, c.max_dv);
            t.sum_abs_dv = t.sum_abs_dv + c.sum_dv;
        }
    }
    if (threadIdx.x == 0) {
        ++t.checks;
        *acc = t;
    }
}

}  // namespace

const char* launch_compare(const CompareArgs& a, long check_index, int fresh, gz_shadow_stats* d_acc, hipStream_t stream) {
    if (a.n < 1 || a.nseg < 1 || a.nseg > kMaxSegments || a.R < 1 || a.R > GZ_MAX_ROLES || !a.rec || !d_acc)
        return "shadow compare: bad arguments";
    int sumP = 0;
    for (int r = 0; r < a.R; ++r) sumP += a.P[r];
    hipLaunchKernelGGL(shadow_row_kernel, dim3((a.n + kRowsPerBlock - 1) / kRowsPerBlock), dim3(64 * kRowsPerBlock), 0, stream, a);
    hipLaunchKernelGGL(shadow_fold_kernel, dim3(1), dim3(kFoldChunk), 0, stream, (const RowRecord*)a.rec, a.n, a.R, sumP, a.V,
                       a.logits, check_index, fresh, d_acc);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace gzshadow
