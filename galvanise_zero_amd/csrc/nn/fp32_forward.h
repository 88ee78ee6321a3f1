// The exact-fp32 forward (GZ_PRECISION_FP32, Python name "fp32-ieee"): the trunk layer by layer
// through HBM on the f32-input MFMA (v_mfma_f32_16x16x4_f32: f32 operands, f32 accumulation -- a
// k-ordered fmaf chain), fp32 activations in a per-stream device scratch, the existing fp32
// heads_kernel on the head features.  fp32_forward.hip holds the kernels; this header holds
//   * the index arithmetic the conv kernel, the weight packing (weight_image.h) and the CPU check
//     (tests/fp32_host_check.cpp) share -- plain C++, usable without a HIP compiler;
//   * the launch interface gz_nn.hip calls (HIP compilers only).
// The layer loop (forward), the scratch and every kernel but the conv and the input gather also serve
// the layered bf16 modes (layered_forward.h, Forward::parts).
//
// The 3x3 conv as an implicit GEMM  out[co][c] = sum_{tap,ci} W[co][tap,ci] * X[nbr(c,tap)][ci]:
// its columns c are the launch's board positions, flat: c = row * npos + p over the NHWC
// activations X[rows * npos][CP].  A workgroup (4 waves) takes kTileCols columns x 32 CT output
// channels; wave w the channel half w & 1 and the column half w >> 1: CT x kWaveTiles accumulator
// tiles of 16 x 16.  Input channels go through the LDS in chunks of kChunk: rows
// [c0 - (W + 1), c0 + kTileCols + (W + 1)) of X (every on-board 3x3 neighbour of the tile's columns;
// rows outside the launch as zeros) plus one all-zero row for off-board neighbours.  Each (chunk,
// tap) is one MFMA chain from zero, added to the column's running total (blocked summation).  Every
// column's k order -- chunk, tap, 16-channel block, MFMA step, the instruction's 4 k -- is fixed by
// the geometry alone, so a board's outputs do not depend on the launch it is part of.
#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#define GZF_HD __host__ __device__
#else
#define GZF_HD
#endif

namespace gzfp32 {

constexpr int kTileCols = 128;    // columns (board positions) per workgroup
constexpr int kWaveTiles = 4;     // 16-column tiles per wave (two waves side by side)
constexpr int kChunk = 64;        // input channels staged per LDS pass
constexpr int kRowPad = 4;        // floats of padding per LDS row (16 lanes' 16-byte reads: 16 bank groups)
constexpr int kMaxBoardSide = 19;

// input channels padded to whole 16-channel k-blocks
GZF_HD inline int pad16(int c) { return (c + 15) & ~15; }

// filters padded to the compiled widths (zero channels); 0: not supported
GZF_HD inline int padded_filters(int F) { return F < 1 ? 0 : F <= 64 ? 64 : F <= 128 ? 128 : F <= 256 ? 256 : 0; }
// 16-channel output tiles per wave: a workgroup covers 32 CT output channels
GZF_HD inline int wave_co_tiles(int FP) { return FP == 64 ? 2 : 4; }

// ---- LDS image of one (tile, chunk) ------------------------------------------------------------
GZF_HD inline int lds_row_stride() { return kChunk + kRowPad; }              // floats
GZF_HD inline int lds_halo(int W) { return W + 1; }                           // rows before / after the tile
GZF_HD inline int lds_zero_row(int W) { return kTileCols + 2 * lds_halo(W); } // the all-zero row (last)
GZF_HD inline int lds_rows(int W) { return lds_zero_row(W) + 1; }
GZF_HD inline size_t lds_bytes(int W) { return (size_t)lds_rows(W) * lds_row_stride() * sizeof(float); }
// flat column staged in LDS row r of the tile starting at column c0 (may lie outside [0, ncols))
GZF_HD inline long lds_row_column(long c0, int W, int r) { return c0 - lds_halo(W) + r; }

// LDS row holding the neighbour at `tap` (0..8, dy = tap / 3 - 1, dx = tap % 3 - 1; a 1x1 conv uses
// tap 4) of the column `tc` of the tile (0 <= tc < kTileCols) at board position p = y W + x; the zero
// row when the neighbour is off the board or the column is past the launch (live == false)
GZF_HD inline int nbr_row(int H, int W, int y, int x, int tap, int tc, bool live) {
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    const bool ok = live && (unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W;
    return ok ? tc + lds_halo(W) + dy * W + dx : lds_zero_row(W);
}

// ---- weights in MFMA A-fragment order ----------------------------------------------------------
// Float offset, within one conv's image, of W[co][tap, ci] (cinp = padded input channels, FP = padded
// filters): [tap][ci / 16][co / 16][lane][step], lane = co % 16 + 16 g, the 16-channel block's channel
// 4 g + step being MFMA step `step`'s k = g.  One wave-wide 16-byte load per (tap, block, co tile)
// reads 1 KB contiguous; the B operand's matching 4 channels are one 16-byte LDS read.
GZF_HD inline size_t wfrag_index(int tap, int co, int ci, int cinp, int FP) {
    const int kb = ci >> 4, g = (ci & 15) >> 2, step = ci & 3;
    const size_t blk = ((size_t)tap * (cinp >> 4) + kb) * (FP >> 4) + (co >> 4);
    return (blk * 64 + (co & 15) + 16 * g) * 4 + step;
}
GZF_HD inline size_t conv_image_floats(int taps, int cinp, int FP) { return (size_t)taps * cinp * FP; }

// ---- device scratch and row chunks -------------------------------------------------------------
// Per row: the gathered input [npos][CP], the ping / pong images and the residual stream
// [npos][FP] each, the squeeze-excite gates [FP]; every buffer starts 256-byte aligned.
GZF_HD inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
struct ScratchLayout {
    size_t in, s, t, x, gate, total;   // byte offsets
};
GZF_HD inline ScratchLayout scratch_layout(int rows, int npos, int CP, int FP) {
    ScratchLayout L{};
    size_t o = 0;
    L.in = o;   o += align256((size_t)rows * npos * CP * 4);
    L.s = o;    o += align256((size_t)rows * npos * FP * 4);
    L.t = o;    o += align256((size_t)rows * npos * FP * 4);
    L.x = o;    o += align256((size_t)rows * npos * FP * 4);
    L.gate = o; o += align256((size_t)rows * FP * 4);
    L.total = o;
    return L;
}
constexpr size_t kScratchMax = (size_t)1 << 30;   // per stream
// rows per sequential chunk of a launch: the most whose scratch stays within kScratchMax (>= 1)
GZF_HD inline int chunk_rows_for(int npos, int CP, int FP) {
    const size_t per_row = (size_t)npos * (CP + 3 * (size_t)FP) * 4 + (size_t)FP * 4;
    size_t r = (kScratchMax - 5 * 256) / per_row;
    if (r < 1) r = 1;
    if (r > (size_t)1 << 20) r = (size_t)1 << 20;
    return (int)r;
}
// chunk i of a launch of n rows: rows [first, first + count)
GZF_HD inline void chunk_bounds(int n, int chunk_rows, int i, int* first, int* count) {
    const long f = (long)i * chunk_rows;
    *first = (int)(f < n ? f : n);
    const long left = (long)n - *first;
    *count = (int)(left < chunk_rows ? left : chunk_rows);
}
GZF_HD inline int chunk_count(int n, int chunk_rows) { return (n + chunk_rows - 1) / chunk_rows; }

}  // namespace gzfp32

// gzfp32::pack_conv_host(dst, w, scale, taps, cin, cinp, F, FP) -- one conv's kernel times scale[co]
// into the zeroed image dst, in wfrag_index order -- comes with the weight packing, whose fp32 conv
// element it loops over.  (weight_image.h includes this header for the index arithmetic above;
// whichever of the two is included first, both are complete after it.)
#include "weight_image.h"

#if defined(__HIPCC__)
#include "forward_kernel.h"

namespace gzfp32 {

// One conv launch of the layer loop
struct ConvArgs {
    const float* x;        // [ncols][cinp]
    const void* w;         // fp32: wfrag_index order; layered: the bf16 / fp16 image (hi parts, or hi | lo fragments)
    const float* bias;     // [FP]
    const float* skip;     // [ncols][FP] added before the activation, or nullptr (may alias out)
    float* out;            // [ncols][FP]
    float* out2;           // v2: act(out * psc + psh), the next block's pre-activation image, or nullptr
    const float* psc;
    const float* psh;
    int ncols, cinp, taps, FP, H, W, npos, act, leaky;
    // the layered modes (layered_forward.h)
    const void* wlo;       // the initial conv's lo image (parts == 3)
    int parts;             // 1: bf16, 3: split, gzlayered::kF16Parts: fp16x3
    int w0_layout;         // w is the initial conv's [K0 / 32][FP][32] image (taps == 1, cinp == K0)
};

// What a launch needs beyond KParams (whose weight pointers b0, bres, wh, bh, wcl, bcl, pre, sew1,
// sew2, segment table and feature scratch it reads as the bf16 kernels do)
struct Forward {
    const float* w0 = nullptr;     // initial conv image [taps0][CP / 16][FP / 16][64][4]
    const float* wres = nullptr;   // trunk conv images [2B][9][FP / 16][FP / 16][64][4]
    int CP = 0, FP = 0;            // input channels of the initial conv's launch (fp32: the planes padded to
                                   // 16; layered: K0, the im2col image's width) / padded filters
    int chunk_rows = 1;            // rows per sequential chunk
    char* scratch = nullptr;       // scratch_layout(scratch_rows, ...) bytes
    int scratch_rows = 0;
    size_t scratch_bytes = 0;
    // The layered modes (layered_forward.h) run the same layer loop with their own conv and input
    // gather: parts = 1 (bf16) or 3 (split), the weights kp.w0 / kp.w0lo / kp.wres; 0: the fp32 conv.
    // parts = gzlayered::kF16Parts: the fp16x3 conv over the fp16 hi | lo image, each conv behind the
    // per-board exponents of its input in bexp (scratch_rows ints, the net's own buffer)
    int parts = 0;
    int* bexp = nullptr;
};

// Queues the trunk of kp.n rows on `stream`: gather, convs, squeeze-excite, the head features into
// kp.feat (heads_kernel follows, launched by the caller).  Returns nullptr, or an error message
// (nothing is launched when a size check fails).
const char* forward(const gznn::KParams& kp, const Forward& f, hipStream_t stream);

// the conv kernel of a net with FP padded filters, as rocprofv3 names it
const char* conv_kernel_name(int FP);

}  // namespace gzfp32
#endif
