// Row-pair geometry of the in-place split kernel at four position tiles (trunk_kernel_h2i<128, 4, 3>,
// 8 x 8 boards only): a position tile (the 16 columns of an MFMA's B operand) is row r of the
// workgroup's board 0 in lanes 0-7 and row r of its board 1 in lanes 8-15.  The workgroup's two wave
// groups become two tile sets, each with rows of both boards: set 0 holds rows 0, 1, 2, 3 as its tiles
// 0-3 and set 1 rows 7, 6, 5, 4, so tile 0 of either set is the one whose 16 lanes all fall off the
// board under three taps (set 0: dy = -1, taps 0-2; set 1: dy = +1, taps 6-8).  Those MFMAs would add
// products with the zero area, +0 or -0, to an fp32 accumulator that started at +0 and so is never
// -0: leaving them out changes no bit of the result -- for finite weights (0 * Inf is NaN).
//
// Plain integer functions for the kernel (forward_kernel.h) and the CPU check
// (tests/h2i_rowpair_host_check.cpp) alike.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GZ_RP_HD __host__ __device__
#else
#define GZ_RP_HD
#endif

namespace gznn {

constexpr int kRowPairSide = 8;                    // H = W = 8
constexpr int kRowPairTiles = 4;                   // position tiles per tile set
constexpr int kRowPairPad = 160;                   // bytes between the two boards' images (rowpair_tap_offset)
// the LDS image of one board as Geo<128, 4, 1, 3, 5> lays it out (checked there): 64 rows of hi | lo
// parts (256 bytes each) + 32 bytes, then two zero rows and a scratch row
constexpr int kRowPairRowBytes = 544, kRowPairHalf = 256, kRowPairImage = 67 * kRowPairRowBytes;
constexpr int kRowPairStride = kRowPairImage + kRowPairPad;

struct RowPairPos {
    int board, pos;    // board of the workgroup (0 / 1), position 8 * row + column
};

// board row of tile t in tile set `set`
GZ_RP_HD constexpr int rowpair_row(int set, int t) { return set == 0 ? t : kRowPairSide - 1 - t; }

// lane li (0-15) of tile t in set `set`
GZ_RP_HD constexpr RowPairPos rowpair_map(int set, int t, int li) {
    return RowPairPos{li >> 3, kRowPairSide * rowpair_row(set, t) + (li & 7)};
}

// the (set, tile, tap) whose MFMAs the looped conv leaves out: every lane's neighbour is off the board
GZ_RP_HD constexpr bool rowpair_skip(int set, int t, int tap) {
    return t == 0 && (set == 0 ? tap < 3 : (tap >= 6 && tap < 9));
}

// LDS byte offset, from board 0's image, of a lane's B fragment (hi part) for tap `tap`, tile t of
// set `set`, k-step 0; k-step kc adds 64 kc, the lo part the row's second half.  ROWS = the padded row
// stride (16-byte slot (2 q + c) mod 16 for chunk c of row q), STRIDE = bytes from board 0's image to
// board 1's.  ds_read_b128 is served in groups of 16 lanes that pair eight positions of one channel
// group with the other eight of the next; the two boards' lanes of a tile keep that group's 16 slots
// distinct only if STRIDE is a multiple of 256.  Off-board neighbours read the zero area behind the
// image's 64 rows at the slot of their virtual position, which depends on the column alone (a board
// row is 8 positions, 16 slots).  The neighbour's row is the same for the tile's 16 lanes, so only the
// column test is per lane.  Tap 9 is the looped conv's read ahead past its last tap, whose values are
// never used: it reads what the centre tap reads.
template <int ROWS, int STRIDE>
GZ_RP_HD inline int rowpair_tap_offset(int set, int t, int lane, int tap) {
    static_assert(STRIDE % 256 == 0, "the two boards' lanes of a tile would share LDS slots");
    const int x = lane & 7, board = (lane >> 3) & 1, g = lane >> 4;
    const int tp = tap > 8 ? 4 : tap;
    const int xx = x + tp % 3 - 1;                      // the neighbour's column
    const int y = rowpair_row(set, t) + tp / 3 - 1;     // and its row
    const bool ok = (unsigned)xx < (unsigned)kRowPairSide && (unsigned)y < (unsigned)kRowPairSide;
    const int a_in = (kRowPairSide * y + xx) * ROWS + (g << 4);
    const int a_zero = kRowPairSide * kRowPairSide * ROWS + (((g + 2 * xx) & 15) << 4);
    return board * STRIDE + (ok ? a_in : a_zero);
}

}  // namespace gznn
