// The layered bf16 forwards (GZ_PRECISION_BF16_LAYERED / GZ_PRECISION_SPLIT_LAYERED, Python names
// "bf16-layered" / "bf16x3-layered"): fp32_forward.h's layer-by-layer trunk -- fp32 NHWC activations
// in the per-stream HBM scratch, every kernel but the conv the fp32 path's own -- with the conv on
// v_mfma_f32_16x16x32_bf16, its operands bf16 (P = 1) or split into bf16 hi + lo (P = 3: hi hi +
// hi lo + lo hi into one fp32 accumulator), the arithmetic of the fused "bf16" / "bf16x3" kernels
// without their whole-net LDS image.  The weights are the fused modes' image, unchanged
// (weight_image.h: wres_index order for the trunk, [K0 / 32][FP][32] for the initial conv).
// layered_forward.hip holds the kernels; this header holds
//   * the index arithmetic the conv kernel and the CPU check (tests/layered_host_check.cpp) share --
//     plain C++, usable without a HIP compiler;
//   * the launch interface fp32_forward.hip's layer loop calls (HIP compilers only).
//
// The conv is fp32_forward.h's implicit GEMM with the same tiling: a workgroup (4 waves) takes
// gzfp32::kTileCols flat columns x 32 CT output channels, input channels go through the LDS in
// chunks of gzfp32::kChunk with the W + 1 halo and the zero row (gzfp32::nbr_row /
// lds_row_column).  The staging loop splits: an LDS row holds the chunk's 64 channels as bf16 hi
// and, for P = 3, 64 bf16 lo behind them (hi = bf16(x) round to nearest even, lo = bf16(x - hi)).
// A k-step is 32 channels: lane (li, g) of a wave reads the 8 channels 8 g .. 8 g + 7 of column
// li's row as one 16-byte B fragment per part.  Every column's order -- chunk, tap, k-step, part
// (hi hi, hi lo, lo hi) -- is fixed by the geometry alone.
//
// The initial conv runs as a 1-tap conv over an im2col image [ncols][K0] (k = tap C + c, zero off
// the board and in the padding to K0), reading the w0 image by w0_frag_index.
//
// GZ_PRECISION_F16X3_LAYERED ("fp16x3-layered", Forward::parts == kF16Parts) is the same path with
// conv_f16_kernel<CT> on v_mfma_f32_16x16x32_f16: the split conv's tiling, LDS rows, fragment
// addresses and image offsets (any 2-byte element), with fp16 parts and a per-board exponent.  For a
// conv with BN-folded weights w and input x, e_b the exponent of the column's board (board_exponent
// of the largest |x| among the board's npos x cinp inputs, written to bexp[row] by board_exp_kernel
// in front of the conv):
//   x^   = x 2^-e_b                       (exact: the board's largest |x^| lies in [2^14, 2^15))
//   x_hi = f16(x^)      x_lo = f16((x^ - x_hi) 2^11)       round to nearest even
//   w_hi = f16(w)       w_lo = f16((w  - w_hi) 2^11)       (weight_image.h f2h / h_lo_of)
//   main += w_hi x_hi ;  corr += w_hi x_lo ;  corr += w_lo x_hi     per k-step, two fp32 accumulators
//   out  = (main + corr 2^-11) 2^e_b      then bias / skip / activation / pre-activation as above
// lo lo is dropped.  The lo parts are scaled so that they stay clear of fp16's subnormals, and summed
// apart so that the scale comes off once.  A 3x3 neighbourhood never leaves its board, so e_b factors
// out of every column; it depends on the board's own data only, so a row's outputs stay independent
// of the launch.  A board with an infinity or a NaN gets e_b = 0 and non-finite outputs.
#pragma once

#include "fp32_forward.h"

namespace gzlayered {

using gzfp32::kChunk;
using gzfp32::kTileCols;
using gzfp32::kWaveTiles;

constexpr int kStep = 32;   // input channels per MFMA (v_mfma_f32_16x16x32_bf16)

constexpr int kF16Parts = 16;   // Forward::parts / P of the fp16x3 conv (1: bf16, 3: bf16 split)

// 2-byte parts per operand of precision P (1, 3 or kF16Parts) = weight_image.h's PackSpec.p2
GZF_HD inline int operand_parts(int P) { return P == 3 || P == kF16Parts ? 2 : 1; }

// ---- LDS image of one (tile, chunk) ------------------------------------------------------------
// Row stride in bytes: 160 (P = 1: 128 of hi + 32) or 288 (P = 3: 128 hi + 128 lo + 32), i.e. 10 or
// 18 sixteen-byte slots.  ds_read_b128 serves a wave in four groups of 16 lanes that are not
// contiguous ({0-3, 12-15, 20-27}, ...): each holds 16 distinct columns li, half of them with the
// k group g and half with g + 1.  The slot (of the 16 in the 256-byte bank row) of column row r,
// group g is (s r + g + const) mod 16 for a stride of s slots; with s = 2 (mod 8) the rows of g
// take the even and those of g + 1 the odd slots, 8 distinct each: conflict-free.  (A stride of 17
// slots, 272 bytes, makes the slot r + g: columns 12, g and 11, g + 1 of one group collide.)
GZF_HD inline int lds_row_bytes(int P) { return (operand_parts(P) * kChunk * 2) + 32; }
GZF_HD inline size_t lds_bytes(int W, int P) { return (size_t)gzfp32::lds_rows(W) * lds_row_bytes(P); }
// byte offset, within an LDS row, of part `part` (0 hi, 1 lo) of chunk channel cc (0 <= cc < kChunk)
GZF_HD inline int lds_channel_offset(int cc, int part) { return part * kChunk * 2 + cc * 2; }
// byte address of the B fragment (8 bf16: chunk channels 32 ks + 8 g ..) lane group g reads for
// k-step ks of the chunk from LDS row `row`
GZF_HD inline int bfrag_addr(int row, int ks, int g, int part, int P) {
    return row * lds_row_bytes(P) + lds_channel_offset(kStep * ks + 8 * g, part);
}

// ---- weights: the fused modes' bf16 images -----------------------------------------------------
// Element offset (bf16) of the 8-element A fragment lane (li = co % 16, g) loads for the trunk conv's
// (tap, k-step kc of 32 input channels, 16-channel output tile cot), part 0 hi / 1 lo:
// = gzw::wres_index(tap, 16 cot + li, 32 kc + 8 g, FP, P2) (+ 512 for lo)
GZF_HD inline size_t wres_frag_index(int tap, int kc, int cot, int li, int g, int part, int FP, int P2) {
    const size_t blk = ((size_t)(tap * (FP >> 5) + kc) * (FP >> 4) + cot) * P2 + part;
    return (blk * 64 + li + 16 * g) * 8;
}
// the same for the initial conv's image [K0 / 32][FP][32] (hi and lo are two images of this layout)
GZF_HD inline size_t w0_frag_index(int kc, int cot, int li, int g, int FP) {
    return (((size_t)kc * FP + 16 * cot + li) * kStep) + 8 * g;
}

// ---- fp16x3: the per-board exponent -------------------------------------------------------------
// e_b from the largest bit pattern of |x| (as unsigned: the order of the magnitudes) among a board's
// inputs: floor(log2(max |x|)) - 14, subnormals included; 0 for an all-zero board and for one holding
// an infinity or a NaN (whose pattern is the largest), which then reaches the outputs as it is.
GZF_HD inline int board_exponent(unsigned maxbits) {
    if (maxbits == 0u || maxbits >= 0x7f800000u) return 0;
    int fl;
    if (maxbits >= 0x00800000u) {
        fl = (int)(maxbits >> 23) - 127;
    } else {
        int top = 22;   // the subnormal's highest set bit
        while (!((maxbits >> top) & 1u)) --top;
        fl = top - 149;
    }
    return fl - 14;
}
constexpr float kF16LoInv = 1.f / 2048.f;   // 2^-11 (gzw::kF16LoScale's inverse)

// ---- the im2col image of the initial conv --------------------------------------------------------
// what element k of a column at board position (y, x) reads: plane *c at (y + *dy, x + *dx); false
// for the padding k >= taps C.  taps = 9 (3x3) or 1 (1x1).
GZF_HD inline bool im2col_source(int k, int C, int taps, int* c, int* dy, int* dx) {
    if (k >= taps * C) return false;
    const int tap = taps == 1 ? 4 : k / C;
    *c = taps == 1 ? k : k - tap * C;
    *dy = tap / 3 - 1;
    *dx = tap % 3 - 1;
    return true;
}

}  // namespace gzlayered

#if defined(__HIPCC__)
namespace gzlayered {

// the conv of fp32_forward.h's layer loop: a.w / a.wlo the bf16 images, a.parts = 1 or 3,
// a.w0_layout set for the initial conv (then a.taps == 1, a.cinp == K0)
const char* launch_conv(const gzfp32::ConvArgs& a, hipStream_t st);
// the segments' planes [rows][C][npos] -> the im2col image [rows * npos][K0]
void launch_im2col(const gznn::KParams& kp, float* in, int row0, int rows, hipStream_t st);
// the conv kernel of a net with FP padded filters and precision P, as rocprofv3 names it
const char* conv_kernel_name(int FP, int P);
// fp16x3: board_exp_kernel over the conv's input (a.ncols / a.npos boards of a.npos x a.cinp values)
// into bexp, then conv_f16_kernel; a.w / a.wlo the fp16 images, a.parts == kF16Parts
const char* launch_conv_f16(const gzfp32::ConvArgs& a, int* bexp, hipStream_t st);

}  // namespace gzlayered
#endif
