// The row-pair geometry of trunk_kernel_h2i<128, 4, 3> (csrc/nn/rowpair.h) checked on the CPU from the
// functions the kernel itself uses:
//   1. (tile set, tile, lane) -> (board, position) is a bijection onto the 2 x 64 positions of a
//      workgroup's two 8 x 8 boards;
//   2. the (set, tile, tap) the looped conv leaves out (rowpair_skip) are exactly those whose 16 lanes
//      all have their neighbour off the board -- no live product is dropped, no dead MFMA kept;
//   3. every B-fragment read (each tap, the read ahead past the last one, k-step, hi and lo part, tile
//      and set) lies in the lane's board's image, on the neighbour's row or wholly inside the zero
//      area, and the 16 addresses of each ds_read_b128 lane group fall into 16 distinct 16-byte slots
//      of the LDS's 256-byte line;
//   4. two workgroups' images, pad and cfg2's bias table fit a CU's LDS.
// Stand-alone: g++ -std=c++17 (tests/test_h2i_rowpair_host_check.py builds it with the sanitizers).
#include "../galvanise_zero_amd/csrc/nn/rowpair.h"

#include <cstdio>
#include <set>
#include <utility>

using namespace gznn;

static int fails = 0;
#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            ++fails;                      \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");            \
        }                                 \
    } while (0)

// ds_read_b128's lane groups on gfx950, one LDS cycle each
static const int kGroups[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63},
};

int main() {
    constexpr int S = kRowPairSide, NPOS = S * S;
    // 1. the map
    std::set<std::pair<int, int>> seen;
    for (int set = 0; set < 2; ++set)
        for (int t = 0; t < kRowPairTiles; ++t)
            for (int li = 0; li < 16; ++li) {
                const RowPairPos m = rowpair_map(set, t, li);
                CHECK(m.board >= 0 && m.board < 2 && m.pos >= 0 && m.pos < NPOS, "map out of range set %d tile %d lane %d", set, t, li);
                CHECK(seen.insert({m.board, m.pos}).second, "map repeats board %d pos %d", m.board, m.pos);
                CHECK(m.pos / S == rowpair_row(set, t), "a tile is one board row: set %d tile %d lane %d", set, t, li);
            }
    CHECK((int)seen.size() == 2 * NPOS, "map covers %d of %d positions", (int)seen.size(), 2 * NPOS);
    std::printf("map: %d positions\n", (int)seen.size());

    // 2. the skipped (set, tile, tap)
    int skipped = 0;
    for (int set = 0; set < 2; ++set)
        for (int t = 0; t < kRowPairTiles; ++t)
            for (int tap = 0; tap < 9; ++tap) {
                bool all_off = true;
                for (int li = 0; li < 16; ++li) {
                    const int p = rowpair_map(set, t, li).pos;
                    const int y = p / S + tap / 3 - 1, x = p % S + tap % 3 - 1;
                    if (y >= 0 && y < S && x >= 0 && x < S) all_off = false;
                }
                CHECK(rowpair_skip(set, t, tap) == all_off, "skip(%d, %d, %d) = %d, all lanes off the board = %d", set, t, tap,
                      (int)rowpair_skip(set, t, tap), (int)all_off);
                skipped += rowpair_skip(set, t, tap);
            }
    CHECK(skipped * 12 == 2 * kRowPairTiles * 9, "skipped %d of %d (1/12 expected)", skipped, 2 * kRowPairTiles * 9);
    CHECK(!rowpair_skip(0, 0, 9) && !rowpair_skip(1, 0, 9), "tap 9 (the next conv's first k-step is read afresh) is no skip");
    std::printf("skipped (set, tile, tap): %d of %d\n", skipped, 2 * kRowPairTiles * 9);

    // 3. the B-fragment reads
    constexpr int ROWS = kRowPairRowBytes, HALF = kRowPairHalf, STRIDE = kRowPairStride;
    constexpr int ZERO0 = NPOS * ROWS, ZERO1 = (NPOS + 2) * ROWS;
    long reads = 0, zero_reads = 0;
    for (int set = 0; set < 2; ++set)
        for (int t = 0; t < kRowPairTiles; ++t)
            for (int tap = 0; tap <= 9; ++tap)
                for (int kc = 0; kc < 4; ++kc)
                    for (int h = 0; h < 2; ++h) {
                        int addr[64];
                        for (int lane = 0; lane < 64; ++lane) {
                            const int a = rowpair_tap_offset<ROWS, STRIDE>(set, t, lane, tap) + 64 * kc + h * HALF;
                            addr[lane] = a;
                            const int li = lane & 15, g = lane >> 4;
                            const RowPairPos m = rowpair_map(set, t, li);
                            const int tp = tap == 9 ? 4 : tap;   // the read ahead: values unused, any valid address
                            const int y = m.pos / S + tp / 3 - 1, x = m.pos % S + tp % 3 - 1;
                            const int img = a - m.board * STRIDE;
                            ++reads;
                            if (y >= 0 && y < S && x >= 0 && x < S) {
                                const int want = (y * S + x) * ROWS + h * HALF + 16 * (4 * kc + g);
                                CHECK(img == want, "set %d tile %d tap %d kc %d h %d lane %d: offset %d, neighbour's chunk at %d", set,
                                      t, tap, kc, h, lane, img, want);
                            } else {
                                ++zero_reads;
                                CHECK(img >= ZERO0 && img + 16 <= ZERO1 && img % 16 == 0,
                                      "set %d tile %d tap %d kc %d h %d lane %d: offset %d outside the zero area [%d, %d)", set, t, tap,
                                      kc, h, lane, img, ZERO0, ZERO1);
                            }
                        }
                        for (int gi = 0; gi < 4; ++gi) {
                            unsigned slots = 0;
                            for (int k = 0; k < 16; ++k) slots |= 1u << ((addr[kGroups[gi][k]] / 16) % 16);
                            CHECK(slots == 0xffffu, "set %d tile %d tap %d kc %d h %d lane group %d: slots %04x", set, t, tap, kc, h, gi,
                                  slots);
                        }
                    }
    std::printf("B-fragment reads: %ld lane addresses, %ld into the zero area, conflict-free\n", reads, zero_reads);

    // 4. the LDS: two images, the pad and a 6-block net's bias table, twice per CU
    constexpr int smem = 2 * kRowPairImage + kRowPairPad + 2 * 6 * 128 * 4;
    CHECK(STRIDE % 256 == 0, "image stride %d is no multiple of 256", STRIDE);
    CHECK(smem == 79200 && 2 * smem <= 160 * 1024, "LDS per workgroup %d", smem);
    std::printf("LDS per workgroup: %d B\n", smem);

    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("h2i row-pair geometry: ok\n");
    return 0;
}
