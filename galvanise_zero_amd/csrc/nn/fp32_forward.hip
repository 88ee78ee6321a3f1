// The exact-fp32 forward's kernels (fp32_forward.h): input gather, the f32-MFMA conv (the one hot
// kernel), squeeze-excite, the head features.  Everything but the conv is plain HIP with one thread
// per output and a sum in fixed order (four interleaved partial sums), no atomics.
#include "fp32_forward.h"
#include "layered_forward.h"

#include <hip/hip_runtime.h>

using namespace gznn;

namespace gzfp32 {
namespace {

// ---- input: the segments' planes [rows][C][npos] -> NHWC [rows * npos][CP] (zero padded channels)
__global__ void __launch_bounds__(256) gather_kernel(const KParams kp, float* in, int row0, int rows, int CP) {
    const int npos = kp.npos, C = kp.C;
    const size_t n = (size_t)rows * npos * CP;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % CP);
        const size_t col = i / CP;
        const int row = (int)(col / npos), p = (int)(col - (size_t)row * npos);
        float v = 0.f;
        if (c < C) {
            const int board = row0 + row;
            const int sg = find_segment(kp, board);
            v = kp.seg[sg].planes[((size_t)(board - kp.seg[sg].row0) * C + c) * npos + p];
        }
        in[i] = v;
    }
}

}  // namespace

// ---- the conv (named gzfp32::conv_f32_kernel<CT>: conv_kernel_name) -------------------------------
template <int CT>
__global__ void __launch_bounds__(256) conv_f32_kernel(const ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int TT = kWaveTiles;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int W = a.W, cinp = a.cinp, FP = a.FP;
    const int stride = lds_row_stride();
    const long c0 = (long)blockIdx.x * kTileCols;
    const int co_wave = (blockIdx.y * 2 + (wave & 1)) * CT * 16;   // the wave's first output channel
    const int tc0 = (wave >> 1) * (TT * 16);                        // its first column within the tile

    // this lane's columns: board coordinates, once
    int ys[TT], xs[TT];
    bool live[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) {
        const long c = c0 + tc0 + 16 * t + li;
        live[t] = c < a.ncols;
        const int p = live[t] ? (int)(c % a.npos) : 0;
        ys[t] = p / W;
        xs[t] = p - ys[t] * W;
    }
    for (int i = tid; i < stride; i += 256) lds[lds_zero_row(W) * stride + i] = 0.f;

    // Blocked summation: each (chunk, tap)'s up to kChunk products form one MFMA chain from zero
    // (acc), added to the running total (tot) -- the rounding error of a K-term serial chain grows
    // like sqrt(K), that of K / 64 blocks of 64 like sqrt(64) + sqrt(K / 64)
    f32x4 acc[CT][TT], tot[CT][TT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int t = 0; t < TT; ++t) tot[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nrows = lds_zero_row(W);   // staged rows (the zero row stays)
    const int cotiles = FP >> 4;
    for (int kc = 0; kc < cinp; kc += kChunk) {
        const int kcl = cinp - kc < kChunk ? cinp - kc : kChunk;   // a multiple of 16
        const int q4 = kcl >> 2;
        __syncthreads();   // the previous chunk's reads are done
        for (int i = tid; i < nrows * q4; i += 256) {
            const int r = i / q4, q = i - r * q4;
            const long f = lds_row_column(c0, W, r);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (f >= 0 && f < a.ncols) v = *(const float4*)(a.x + (size_t)f * cinp + kc + 4 * q);
            *(float4*)(lds + r * stride + 4 * q) = v;
        }
        __syncthreads();
        const int nkb = kcl >> 4;
        for (int tp = 0; tp < a.taps; ++tp) {
            const int tap = a.taps == 1 ? 4 : tp;
            int row[TT];
#pragma unroll
            for (int t = 0; t < TT; ++t) row[t] = nbr_row(a.H, W, ys[t], xs[t], tap, tc0 + 16 * t + li, live[t]) * stride + 4 * g;
            const float* wt = (const float*)a.w + (((size_t)tp * (cinp >> 4) + (kc >> 4)) * cotiles + (co_wave >> 4)) * 256 + 4 * lane;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int t = 0; t < TT; ++t) acc[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int kb = 0; kb < nkb; ++kb) {
                float4 af[CT], bf[TT];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) af[ct] = *(const float4*)(wt + ((size_t)kb * cotiles + ct) * 256);
#pragma unroll
                for (int t = 0; t < TT; ++t) bf[t] = *(const float4*)(lds + row[t] + 16 * kb);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int t = 0; t < TT; ++t) acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ct].x, bf[t].x, acc[ct][t], 0, 0, 0);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int t = 0; t < TT; ++t) acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ct].y, bf[t].y, acc[ct][t], 0, 0, 0);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int t = 0; t < TT; ++t) acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ct].z, bf[t].z, acc[ct][t], 0, 0, 0);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int t = 0; t < TT; ++t) acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ct].w, bf[t].w, acc[ct][t], 0, 0, 0);
            }
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int t = 0; t < TT; ++t) tot[ct][t] += acc[ct][t];
        }
    }

    // epilogue: accumulator register i of lane (li, g) is channel 4 g + i of its tile, column li
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int co = co_wave + 16 * ct + 4 * g;
        const float4 bias = *(const float4*)(a.bias + co);
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.out2) {
            sc = *(const float4*)(a.psc + co);
            sh = *(const float4*)(a.psh + co);
        }
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            if (!live[t]) continue;
            const size_t o = (size_t)(c0 + tc0 + 16 * t + li) * FP + co;
            f32x4 v = tot[ct][t];
            v[0] += bias.x; v[1] += bias.y; v[2] += bias.z; v[3] += bias.w;
            if (a.skip) {
                const float4 r = *(const float4*)(a.skip + o);
                v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
            }
            if (a.act) {
                v[0] = act_fn(v[0], a.leaky);
                v[1] = act_fn(v[1], a.leaky);
                v[2] = act_fn(v[2], a.leaky);
                v[3] = act_fn(v[3], a.leaky);
            }
            *(float4*)(a.out + o) = make_float4(v[0], v[1], v[2], v[3]);
            if (a.out2) {
                const f32x4 pv = pre_act(v, sc, sh, a.leaky);
                *(float4*)(a.out2 + o) = make_float4(pv[0], pv[1], pv[2], pv[3]);
            }
        }
    }
}

namespace {
// Sums in a fixed order with four interleaved partial sums (element i into partial i % 4, then
// (s0 + s1) + (s2 + s3)): a quarter of a serial chain's length per partial
__device__ __forceinline__ float sum4(const float* x, int n, int stride) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int i = 0;
    for (; i + 4 <= n; i += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += x[(size_t)(i + k) * stride];
    }
    for (int k = 0; i < n; ++i, ++k) s[k] += x[(size_t)i * stride];
    return (s[0] + s[1]) + (s[2] + s[3]);
}
__device__ __forceinline__ float dot4(const float* x, int xs, const float* w, int ws, int n) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int i = 0;
    for (; i + 4 <= n; i += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += x[(size_t)(i + k) * xs] * w[(size_t)(i + k) * ws];
    }
    for (int k = 0; i < n; ++i, ++k) s[k] += x[(size_t)i * xs] * w[(size_t)i * ws];
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// ---- squeeze-excite (model.py:101-126): channel means -> Dense(S) relu -> Dense(F) sigmoid --------
// one workgroup of FP threads per row; u = conv2 + bias [rows * npos][FP]
__global__ void __launch_bounds__(256) se_gate_kernel(const float* u, const float* w1, const float* w2, float* gate,
                                                      int npos, int FP, int S) {
    __shared__ float mean[256];
    __shared__ float hid[kMaxSE];
    const int row = blockIdx.x, c = threadIdx.x;
    const float* ur = u + (size_t)row * npos * FP;
    mean[c] = sum4(ur + c, npos, FP) * (1.f / (float)npos);
    __syncthreads();
    for (int j = c; j < S; j += FP) {   // (S may exceed a narrow net's FP threads)
        hid[j] = fmaxf(dot4(mean, 1, w1 + j, S, FP), 0.f);
    }
    __syncthreads();
    float z = 0.f;
    for (int j = 0; j < S; ++j) z += hid[j] * w2[(size_t)j * FP + c];
    gate[(size_t)row * FP + c] = 1.f / (1.f + expf(-z));
}

// stream s += u * gate; x = act(s * psc + psh) when another block follows (in place on u)
__global__ void __launch_bounds__(256) se_apply_kernel(float* s, float* x, const float* gate, const float* psc,
                                                       const float* psh, int rows, int npos, int FP, int more, int leaky) {
    const int f4 = FP >> 2;
    const size_t n = (size_t)rows * npos * f4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % f4) * 4;
        const int row = (int)(i / ((size_t)npos * f4));
        const float4 gt = *(const float4*)(gate + (size_t)row * FP + c);
        const float4 uv = ((const float4*)x)[i];
        const float4 sv = ((const float4*)s)[i];
        const float m0 = uv.x * gt.x, m1 = uv.y * gt.y, m2 = uv.z * gt.z, m3 = uv.w * gt.w;
        f32x4 v = {sv.x + m0, sv.y + m1, sv.z + m2, sv.w + m3};
        ((float4*)s)[i] = make_float4(v[0], v[1], v[2], v[3]);
        if (more) {
            const f32x4 pv = pre_act(v, *(const float4*)(psc + c), *(const float4*)(psh + c), leaky);
            ((float4*)x)[i] = make_float4(pv[0], pv[1], pv[2], pv[3]);
        }
    }
}

// ---- head features into kp.feat, the [n][FS] layout heads_kernel reads ----------------------------
// the heads' 1x1 convs (BN folded) of the trunk output s: one thread per (column, conv)
__global__ void __launch_bounds__(256) head_conv_kernel(const KParams kp, const float* s, int row0, int rows, int FP) {
    const int npos = kp.npos, HC = 2 * kp.R + (kp.cal ? 0 : 1);
    const size_t n = (size_t)rows * npos * HC;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int h = (int)(i % HC);
        const size_t col = i / HC;
        const int row = (int)(col / npos), p = (int)(col - (size_t)row * npos);
        const float* sr = s + col * FP;
        const float* w = kp.wh + (size_t)h * FP;
        const float sum = act_fn(dot4(sr, 1, w, 1, FP) + kp.bh[h], kp.leaky);
        float* f = kp.feat + (size_t)(row0 + row) * kp.FS;
        if (h < 2 * kp.R) {
            const int r = h >> 1, ch = h & 1;
            f[r * 2 * npos + (kp.flatten_nchw ? ch * npos + p : p * 2 + ch)] = sum;
        } else {
            f[2 * kp.R * npos + kp.gapF + p] = sum;
        }
    }
}

// concat_all_layers: trunk layer j's value conv (model.py:251-260)
__global__ void __launch_bounds__(256) layer_conv_kernel(const KParams kp, const float* s, int row0, int rows, int FP, int j) {
    const int npos = kp.npos;
    const size_t n = (size_t)rows * npos;
    for (size_t col = (size_t)blockIdx.x * blockDim.x + threadIdx.x; col < n; col += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(col / npos), p = (int)(col - (size_t)row * npos);
        const float* sr = s + col * FP;
        const float* w = kp.wcl + (size_t)j * FP;
        kp.feat[(size_t)(row0 + row) * kp.FS + 2 * kp.R * npos + j * npos + p] = act_fn(dot4(sr, 1, w, 1, FP) + kp.bcl[j], kp.leaky);
    }
}

// pooling value head: the trunk's channel means (model.py:263)
__global__ void __launch_bounds__(256) gap_kernel(const KParams kp, const float* s, int row0, int rows, int FP) {
    const int npos = kp.npos, G = kp.gapF;
    const size_t n = (size_t)rows * G;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % G), row = (int)(i / G);
        const float* sr = s + (size_t)row * npos * FP + c;
        kp.feat[(size_t)(row0 + row) * kp.FS + 2 * kp.R * npos + c] = sum4(sr, npos, FP) * (1.f / (float)npos);
    }
}

unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256 < 65535 ? (n + 255) / 256 : 65535); }

const char* launch_conv(const ConvArgs& a, hipStream_t st) {
    const int CT = wave_co_tiles(a.FP);
    if (a.ncols < 1 || a.cinp < 16 || (a.cinp & 15) || a.FP % (32 * CT) != 0 || (a.taps != 1 && a.taps != 9))
        return "fp32 conv: bad shape";
    const dim3 grid((unsigned)((a.ncols + kTileCols - 1) / kTileCols), (unsigned)(a.FP / (32 * CT)));
    const size_t smem = lds_bytes(a.W);
    if (CT == 2) hipLaunchKernelGGL(conv_f32_kernel<2>, grid, dim3(256), smem, st, a);
    else hipLaunchKernelGGL(conv_f32_kernel<4>, grid, dim3(256), smem, st, a);
    return nullptr;
}

}  // namespace

const char* conv_kernel_name(int FP) {
    return wave_co_tiles(FP) == 2 ? "gzfp32::conv_f32_kernel<2>" : "gzfp32::conv_f32_kernel<4>";
}

const char* forward(const KParams& kp, const Forward& f, hipStream_t st) {
    const int npos = kp.npos, FP = f.FP, CP = f.CP, B = kp.B;
    // every size the kernels rely on, before anything is launched
    if (kp.n < 1) return nullptr;
    const bool layered = f.parts != 0;   // the conv and the input gather of layered_forward.h
    const bool f16 = f.parts == gzlayered::kF16Parts;   // conv_f16_kernel behind board_exp_kernel
    if (layered && f.parts != 1 && f.parts != 3 && !f16) return "fp32 forward: bad part count";
    if (layered ? (!kp.w0 || (f.parts != 1 && !kp.w0lo) || (B > 0 && !kp.wres)) : (!f.w0 || (B > 0 && !f.wres)))
        return "fp32 forward: missing weights";
    if (!f.scratch || !kp.feat || (f16 && !f.bexp)) return "fp32 forward: missing buffer";
    if (kp.H < 1 || kp.W < 1 || kp.H > kMaxBoardSide || kp.W > kMaxBoardSide || npos != kp.H * kp.W)
        return "fp32 forward: board out of range";
    if (padded_filters(FP) != FP || CP != (layered ? kp.K0 : pad16(kp.C)) || FP > 256 || kp.S > kMaxSE)
        return "fp32 forward: channel counts out of range";
    if (f.chunk_rows < 1 || f.scratch_rows < (kp.n < f.chunk_rows ? kp.n : f.chunk_rows))
        return "fp32 forward: scratch rows too few";
    if ((size_t)f.scratch_rows * npos > ((size_t)1 << 31) / 260) return "fp32 forward: chunk too large";
    const ScratchLayout L = scratch_layout(f.scratch_rows, npos, CP, FP);
    if (L.total > f.scratch_bytes) return "fp32 forward: scratch too small";
    if ((layered ? gzlayered::lds_bytes(kp.W, f.parts) : lds_bytes(kp.W)) > 64 * 1024) return "fp32 forward: LDS image too large";
    float* in = (float*)(f.scratch + L.in);
    float* S = (float*)(f.scratch + L.s);
    float* T = (float*)(f.scratch + L.t);
    float* X = (float*)(f.scratch + L.x);
    float* gate = (float*)(f.scratch + L.gate);
    const bool v2 = kp.v2 != 0;
    // one trunk conv's image: fp32 in wfrag_index order, or the fused modes' bf16 fragments (hi | lo)
    const char* wres = layered ? (const char*)kp.wres : (const char*)f.wres;
    const size_t conv_bytes = layered ? (size_t)gzlayered::operand_parts(f.parts) * 9 * FP * FP * 2 : conv_image_floats(9, FP, FP) * 4;

    for (int ck = 0; ck < chunk_count(kp.n, f.chunk_rows); ++ck) {
        int row0, rows;
        chunk_bounds(kp.n, f.chunk_rows, ck, &row0, &rows);
        if (rows < 1 || rows > f.scratch_rows) return "fp32 forward: chunk bounds";
        const int ncols = rows * npos;
        if (layered) gzlayered::launch_im2col(kp, in, row0, rows, st);
        else hipLaunchKernelGGL(gather_kernel, dim3(blocks_for((size_t)ncols * CP)), dim3(256), 0, st, kp, in, row0, rows, CP);
        ConvArgs a{};
        a.parts = f.parts;
        a.ncols = ncols; a.FP = FP; a.H = kp.H; a.W = kp.W; a.npos = npos; a.leaky = kp.leaky;
        auto conv = [&](const float* x, const void* w, const float* bias, int cinp, int taps, const float* skip, float* out,
                        int act, float* out2, int pre_blk) {
            a.x = x; a.w = w; a.bias = bias; a.cinp = cinp; a.taps = taps; a.skip = skip; a.out = out; a.act = act;
            a.out2 = out2;
            a.psc = out2 ? kp.pre + (size_t)(2 * pre_blk) * FP : nullptr;
            a.psh = out2 ? kp.pre + (size_t)(2 * pre_blk + 1) * FP : nullptr;
            if (f16) return gzlayered::launch_conv_f16(a, f.bexp, st);
            return layered ? gzlayered::launch_conv(a, st) : launch_conv(a, st);
        };
        const char* e;
        // initial conv: the stream s (v1: activated; v2: + the first block's pre-activation image)
        // (layered: a 1-tap conv over the im2col image, its weights the [K0 / 32][FP][32] image)
        a.w0_layout = layered ? 1 : 0;
        a.wlo = layered ? kp.w0lo : nullptr;
        e = conv(in, layered ? (const void*)kp.w0 : (const void*)f.w0, kp.b0, CP, layered ? 1 : kp.k0taps, nullptr, S,
                 (!v2 || kp.init_act) ? 1 : 0, (v2 && B > 0) ? X : nullptr, 0);
        a.w0_layout = 0;
        a.wlo = nullptr;
        if (e) return e;
        if (kp.cal) hipLaunchKernelGGL(layer_conv_kernel, dim3(blocks_for(ncols)), dim3(256), 0, st, kp, S, row0, rows, FP, 0);
        for (int blk = 0; blk < B; ++blk) {
            const char* w1 = wres + (size_t)(2 * blk) * conv_bytes;
            const char* w2 = w1 + conv_bytes;
            const float* b1 = kp.bres + (size_t)(2 * blk) * FP;
            const float* b2 = b1 + FP;
            if (!v2) {   // s = act(conv2(act(conv1(s))) + s)
                if ((e = conv(S, w1, b1, FP, 9, nullptr, T, 1, nullptr, 0))) return e;
                if ((e = conv(T, w2, b2, FP, 9, S, S, 1, nullptr, 0))) return e;
                continue;
            }
            const bool more = blk + 1 < B;
            if ((e = conv(X, w1, b1, FP, 9, nullptr, T, 1, nullptr, 0))) return e;
            if (kp.S) {   // s += gate * (conv2 + bias)
                if ((e = conv(T, w2, b2, FP, 9, nullptr, X, 0, nullptr, 0))) return e;
                hipLaunchKernelGGL(se_gate_kernel, dim3(rows), dim3(FP), 0, st, X, kp.sew1 + (size_t)blk * FP * kp.S,
                                   kp.sew2 + (size_t)blk * kp.S * FP, gate, npos, FP, kp.S);
                hipLaunchKernelGGL(se_apply_kernel, dim3(blocks_for((size_t)ncols * (FP >> 2))), dim3(256), 0, st, S, X, gate,
                                   kp.pre + (size_t)(more ? 2 * blk + 2 : 0) * FP, kp.pre + (size_t)(more ? 2 * blk + 3 : 0) * FP,
                                   rows, npos, FP, more ? 1 : 0, kp.leaky);
            } else {
                if ((e = conv(T, w2, b2, FP, 9, S, S, 0, more ? X : nullptr, blk + 1))) return e;
            }
            if (kp.cal)
                hipLaunchKernelGGL(layer_conv_kernel, dim3(blocks_for(ncols)), dim3(256), 0, st, kp, S, row0, rows, FP, blk + 1);
        }
        const int HC = 2 * kp.R + (kp.cal ? 0 : 1);
        hipLaunchKernelGGL(head_conv_kernel, dim3(blocks_for((size_t)ncols * HC)), dim3(256), 0, st, kp, S, row0, rows, FP);
        if (kp.gapF) hipLaunchKernelGGL(gap_kernel, dim3(blocks_for((size_t)rows * kp.gapF)), dim3(256), 0, st, kp, S, row0, rows, FP);
    }
    return hipGetLastError() == hipSuccess ? nullptr : "fp32 forward: kernel launch failed";
}

}  // namespace gzfp32
