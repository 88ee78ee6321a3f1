// The layered bf16 forwards' kernels (layered_forward.h): the conv of fp32_forward.hip's layer loop on
// v_mfma_f32_16x16x32_bf16 (the one hot kernel) and the im2col gather in front of the initial conv.
// Every other kernel of these modes' trunk is fp32_forward.hip's.  "fp16x3-layered" adds its conv on
// v_mfma_f32_16x16x32_f16 (conv_f16_kernel) and the per-board exponent in front of it (board_exp_kernel).
#include "layered_forward.h"

#include <hip/hip_runtime.h>

using namespace gznn;

namespace gzlayered {

using gzfp32::ConvArgs;
using gzfp32::lds_row_column;
using gzfp32::lds_zero_row;
using gzfp32::nbr_row;

namespace {

// ---- input: the segments' planes [rows][C][npos] -> the initial conv's im2col image [rows * npos][K0]
__global__ void __launch_bounds__(256) im2col_kernel(const KParams kp, float* in, int row0, int rows) {
    const int npos = kp.npos, C = kp.C, K0 = kp.K0, H = kp.H, W = kp.W;
    const size_t n = (size_t)rows * npos * K0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % K0);
        const size_t col = i / K0;
        const int row = (int)(col / npos), p = (int)(col - (size_t)row * npos);
        float v = 0.f;
        int c, dy, dx;
        if (im2col_source(k, C, kp.k0taps, &c, &dy, &dx)) {
            const int y = p / W + dy, x = p % W + dx;
            if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
                const int board = row0 + row;
                const int sg = find_segment(kp, board);
                v = kp.seg[sg].planes[((size_t)(board - kp.seg[sg].row0) * C + c) * npos + y * W + x];
            }
        }
        in[i] = v;
    }
}

// ---- fp16x3: bexp[board] = board_exponent(largest |x| pattern of the board's n4 x 4 inputs); one
// workgroup per board
__global__ void __launch_bounds__(256) board_exp_kernel(const float* x, int* bexp, int n4) {
    __shared__ unsigned red[4];
    const uint4* src = (const uint4*)x + (size_t)blockIdx.x * n4;
    unsigned m = 0u;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const uint4 v = src[i];
        const unsigned a = max(v.x & 0x7fffffffu, v.y & 0x7fffffffu), b = max(v.z & 0x7fffffffu, v.w & 0x7fffffffu);
        m = max(m, max(a, b));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) bexp[blockIdx.x] = board_exponent(max(max(red[0], red[1]), max(red[2], red[3])));
}

}  // namespace

// ---- the conv (named gzlayered::conv_bf16_kernel<CT, P>: conv_kernel_name) ------------------------
template <int CT, int P>
__global__ void __launch_bounds__(256) conv_bf16_kernel(const ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int TT = kWaveTiles, NP = P == 3 ? 2 : 1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int W = a.W, cinp = a.cinp, FP = a.FP;
    const int stride = lds_row_bytes(P);
    const long c0 = (long)blockIdx.x * kTileCols;
    const int cot0 = (blockIdx.y * 2 + (wave & 1)) * CT;   // the wave's first 16-channel output tile
    const int tc0 = (wave >> 1) * (TT * 16);               // its first column within the tile

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
    for (int i = tid; i < stride / 4; i += 256) *(uint32_t*)(lds + lds_zero_row(W) * stride + 4 * i) = 0u;

    // one fp32 accumulator per output: chunk, tap, k-step, part in this order
    f32x4 acc[CT][TT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int t = 0; t < TT; ++t) acc[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // A fragments: element strides per k-step and per output tile of the image at hand; the lo
    // fragment sits 512 elements behind the hi one (trunk) or in the lo image (initial conv)
    const __bf16* const wbase = (const __bf16*)a.w;
    const __bf16* const wlbase = a.w0_layout ? (const __bf16*)a.wlo : wbase;
    const size_t ks_stride = a.w0_layout ? w0_frag_index(1, 0, 0, 0, FP) : wres_frag_index(0, 1, 0, 0, 0, 0, FP, NP);
    const size_t ct_stride = a.w0_layout ? w0_frag_index(0, 1, 0, 0, FP) : wres_frag_index(0, 0, 1, 0, 0, 0, FP, NP);

    const int nrows = lds_zero_row(W);   // staged rows (the zero row stays)
    for (int kc = 0; kc < cinp; kc += kChunk) {
        const int kcl = cinp - kc < kChunk ? cinp - kc : kChunk;   // a multiple of kStep
        const int q8 = kcl >> 3;
        __syncthreads();   // the previous chunk's reads are done
        // staging: 8 channels per thread and pass, split into bf16 hi (round to nearest even) and
        // lo = bf16(x - hi), one 16-byte store per part
        for (int i = tid; i < nrows * q8; i += 256) {
            const int r = i / q8, q = i - r * q8;
            const long f = lds_row_column(c0, W, r);
            float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (f >= 0 && f < a.ncols) {
                const float4* src = (const float4*)(a.x + (size_t)f * cinp + kc + 8 * q);
                const float4 v0 = src[0], v1 = src[1];
                x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w;
                x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
            }
            bf16x8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                hi[e] = (__bf16)x[e];
                lo[e] = (__bf16)(x[e] - (float)hi[e]);
            }
            *(bf16x8*)(lds + r * stride + lds_channel_offset(8 * q, 0)) = hi;
            if (P == 3) *(bf16x8*)(lds + r * stride + lds_channel_offset(8 * q, 1)) = lo;
        }
        __syncthreads();
        const int nks = kcl >> 5;
        for (int tp = 0; tp < a.taps; ++tp) {
            const int tap = a.taps == 1 ? 4 : tp;
            int row[TT];
#pragma unroll
            for (int t = 0; t < TT; ++t)
                row[t] = bfrag_addr(nbr_row(a.H, W, ys[t], xs[t], tap, tc0 + 16 * t + li, live[t]), 0, g, 0, P);
            const size_t wo = a.w0_layout ? w0_frag_index(kc >> 5, cot0, li, g, FP) : wres_frag_index(tp, kc >> 5, cot0, li, g, 0, FP, NP);
            const __bf16* wh = wbase + wo;
            const __bf16* wl = wlbase + wo + (a.w0_layout ? 0 : 512);
            for (int ks = 0; ks < nks; ++ks) {
                bf16x8 ah[CT], al[CT], bh[TT], bl[TT];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    ah[ct] = *(const bf16x8*)(wh + ks * ks_stride + ct * ct_stride);
                    if (P == 3) al[ct] = *(const bf16x8*)(wl + ks * ks_stride + ct * ct_stride);
                }
#pragma unroll
                for (int t = 0; t < TT; ++t) {
                    bh[t] = *(const bf16x8*)(lds + row[t] + 2 * kStep * ks);
                    if (P == 3) bl[t] = *(const bf16x8*)(lds + row[t] + 2 * kStep * ks + 2 * kChunk);
                }
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int t = 0; t < TT; ++t) acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[ct], bh[t], acc[ct][t], 0, 0, 0);
                if (P == 3) {
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                        for (int t = 0; t < TT; ++t) acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[ct], bl[t], acc[ct][t], 0, 0, 0);
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                        for (int t = 0; t < TT; ++t) acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[ct], bh[t], acc[ct][t], 0, 0, 0);
                }
            }
        }
    }

    // epilogue (conv_f32_kernel's): accumulator register i of lane (li, g) is channel 4 g + i of its
    // tile, column li
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int co = 16 * (cot0 + ct) + 4 * g;
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
            f32x4 v = acc[ct][t];
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

// ---- the fp16x3 conv (named gzlayered::conv_f16_kernel<CT>): conv_bf16_kernel<CT, 3> with fp16 parts,
// the staged rows scaled by their board's exponent, and two accumulator sets (main: hi hi; corr: hi lo
// + lo hi, whose lo parts carry 2^11) -- the arithmetic of layered_forward.h
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

template <int CT>
__global__ void __launch_bounds__(256, 2) conv_f16_kernel(const ConvArgs a, const int* __restrict__ bexp) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int TT = kWaveTiles, P = kF16Parts, NP = 2;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int W = a.W, cinp = a.cinp, FP = a.FP;
    const int stride = lds_row_bytes(P);
    const long c0 = (long)blockIdx.x * kTileCols;
    const int cot0 = (blockIdx.y * 2 + (wave & 1)) * CT;   // the wave's first 16-channel output tile
    const int tc0 = (wave >> 1) * (TT * 16);               // its first column within the tile

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
    for (int i = tid; i < stride / 4; i += 256) *(uint32_t*)(lds + lds_zero_row(W) * stride + 4 * i) = 0u;

    // two fp32 accumulators per output: chunk, tap, k-step, part in this order
    f32x4 acc[CT][TT], cor[CT][TT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int t = 0; t < TT; ++t) acc[ct][t] = cor[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // A fragments: as conv_bf16_kernel's (the lo fragment 512 elements behind the hi one, or in the lo image)
    const _Float16* const wbase = (const _Float16*)a.w;
    const _Float16* const wlbase = a.w0_layout ? (const _Float16*)a.wlo : wbase;
    const size_t ks_stride = a.w0_layout ? w0_frag_index(1, 0, 0, 0, FP) : wres_frag_index(0, 1, 0, 0, 0, 0, FP, NP);
    const size_t ct_stride = a.w0_layout ? w0_frag_index(0, 1, 0, 0, FP) : wres_frag_index(0, 0, 1, 0, 0, 0, FP, NP);

    const int nrows = lds_zero_row(W);   // staged rows (the zero row stays)
    for (int kc = 0; kc < cinp; kc += kChunk) {
        const int kcl = cinp - kc < kChunk ? cinp - kc : kChunk;   // a multiple of kStep
        const int q8 = kcl >> 3;
        __syncthreads();   // the previous chunk's reads are done
        // staging: 8 channels per thread and pass, scaled by 2^-e of the row's board (flat column /
        // npos), split into fp16 hi (round to nearest even) and lo = fp16((x - hi) 2^11), one 16-byte
        // store per part; rows outside the launch stay zero
        for (int i = tid; i < nrows * q8; i += 256) {
            const int r = i / q8, q = i - r * q8;
            const long f = lds_row_column(c0, W, r);
            float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            int eb = 0;
            if (f >= 0 && f < a.ncols) {
                const float4* src = (const float4*)(a.x + (size_t)f * cinp + kc + 8 * q);
                const float4 v0 = src[0], v1 = src[1];
                x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w;
                x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
                eb = bexp[(int)f / a.npos];
            }
            f16x8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float s = ldexpf(x[e], -eb);
                hi[e] = (_Float16)s;
                lo[e] = (_Float16)((s - (float)hi[e]) * gzw::kF16LoScale);
            }
            *(f16x8*)(lds + r * stride + lds_channel_offset(8 * q, 0)) = hi;
            *(f16x8*)(lds + r * stride + lds_channel_offset(8 * q, 1)) = lo;
        }
        __syncthreads();
        const int nks = kcl >> 5;
        for (int tp = 0; tp < a.taps; ++tp) {
            const int tap = a.taps == 1 ? 4 : tp;
            int row[TT];
#pragma unroll
            for (int t = 0; t < TT; ++t)
                row[t] = bfrag_addr(nbr_row(a.H, W, ys[t], xs[t], tap, tc0 + 16 * t + li, live[t]), 0, g, 0, P);
            const size_t wo = a.w0_layout ? w0_frag_index(kc >> 5, cot0, li, g, FP) : wres_frag_index(tp, kc >> 5, cot0, li, g, 0, FP, NP);
            const _Float16* wh = wbase + wo;
            const _Float16* wl = wlbase + wo + (a.w0_layout ? 0 : 512);
            for (int ks = 0; ks < nks; ++ks) {
                f16x8 ah[CT], al[CT], bh[TT], bl[TT];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    ah[ct] = *(const f16x8*)(wh + ks * ks_stride + ct * ct_stride);
                    al[ct] = *(const f16x8*)(wl + ks * ks_stride + ct * ct_stride);
                }
#pragma unroll
                for (int t = 0; t < TT; ++t) {
                    bh[t] = *(const f16x8*)(lds + row[t] + 2 * kStep * ks);
                    bl[t] = *(const f16x8*)(lds + row[t] + 2 * kStep * ks + 2 * kChunk);
                }
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int t = 0; t < TT; ++t) acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[ct], bh[t], acc[ct][t], 0, 0, 0);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int t = 0; t < TT; ++t) cor[ct][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[ct], bl[t], cor[ct][t], 0, 0, 0);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int t = 0; t < TT; ++t) cor[ct][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[ct], bh[t], cor[ct][t], 0, 0, 0);
            }
        }
    }

    // epilogue: out = (main + corr 2^-11) 2^e of the column's board, then conv_bf16_kernel's
    int es[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) es[t] = live[t] ? bexp[(int)(c0 + tc0 + 16 * t + li) / a.npos] : 0;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int co = 16 * (cot0 + ct) + 4 * g;
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
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = ldexpf(acc[ct][t][i] + cor[ct][t][i] * kF16LoInv, es[t]);
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

const char* launch_conv_f16(const ConvArgs& a, int* bexp, hipStream_t st) {
    const int CT = gzfp32::wave_co_tiles(a.FP);
    if (a.ncols < 1 || a.npos < 1 || a.ncols % a.npos != 0 || a.cinp < kStep || (a.cinp % kStep) || a.FP % (32 * CT) != 0 ||
        (a.taps != 1 && a.taps != 9) || a.parts != kF16Parts || !a.w || !bexp || (a.w0_layout && (a.taps != 1 || !a.wlo)) ||
        (!a.w0_layout && a.cinp != a.FP))
        return "layered conv: bad shape";
    hipLaunchKernelGGL(board_exp_kernel, dim3((unsigned)(a.ncols / a.npos)), dim3(256), 0, st, a.x, bexp, a.npos * a.cinp / 4);
    const dim3 grid((unsigned)((a.ncols + kTileCols - 1) / kTileCols), (unsigned)(a.FP / (32 * CT)));
    const size_t smem = lds_bytes(a.W, kF16Parts);
    if (CT == 2) hipLaunchKernelGGL(conv_f16_kernel<2>, grid, dim3(256), smem, st, a, (const int*)bexp);
    else hipLaunchKernelGGL(conv_f16_kernel<4>, grid, dim3(256), smem, st, a, (const int*)bexp);
    return nullptr;
}

const char* launch_conv(const ConvArgs& a, hipStream_t st) {
    const int CT = gzfp32::wave_co_tiles(a.FP);
    if (a.ncols < 1 || a.cinp < kStep || (a.cinp % kStep) || a.FP % (32 * CT) != 0 || (a.taps != 1 && a.taps != 9) ||
        (a.parts != 1 && a.parts != 3) || !a.w || (a.w0_layout && (a.taps != 1 || (a.parts == 3 && !a.wlo))) ||
        (!a.w0_layout && a.cinp != a.FP))
        return "layered conv: bad shape";
    const dim3 grid((unsigned)((a.ncols + kTileCols - 1) / kTileCols), (unsigned)(a.FP / (32 * CT)));
    const size_t smem = lds_bytes(a.W, a.parts);
    if (a.parts == 1) {
        if (CT == 2) hipLaunchKernelGGL((conv_bf16_kernel<2, 1>), grid, dim3(256), smem, st, a);
        else hipLaunchKernelGGL((conv_bf16_kernel<4, 1>), grid, dim3(256), smem, st, a);
    } else {
        if (CT == 2) hipLaunchKernelGGL((conv_bf16_kernel<2, 3>), grid, dim3(256), smem, st, a);
        else hipLaunchKernelGGL((conv_bf16_kernel<4, 3>), grid, dim3(256), smem, st, a);
    }
    return nullptr;
}

void launch_im2col(const KParams& kp, float* in, int row0, int rows, hipStream_t st) {
    const size_t n = (size_t)rows * kp.npos * kp.K0;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 65535 ? (n + 255) / 256 : 65535);
    hipLaunchKernelGGL(im2col_kernel, dim3(blocks), dim3(256), 0, st, kp, in, row0, rows);
}

const char* conv_kernel_name(int FP, int P) {
    const bool two = gzfp32::wave_co_tiles(FP) == 2;
    if (P == kF16Parts) return two ? "gzlayered::conv_f16_kernel<2>" : "gzlayered::conv_f16_kernel<4>";
    if (P == 3) return two ? "gzlayered::conv_bf16_kernel<2, 3>" : "gzlayered::conv_bf16_kernel<4, 3>";
    return two ? "gzlayered::conv_bf16_kernel<2, 1>" : "gzlayered::conv_bf16_kernel<4, 1>";
}

}  // namespace gzlayered
