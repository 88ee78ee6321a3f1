// Stand-alone CPU check of the one-symmetry-per-row definition in csrc/nn/symmetry.h (built with
// -fsanitize=address,undefined by tests/test_symmetry_pick.py): the row hash and the pick, the expand
// kernel's index arithmetic and the gather kernel's (segment lookup included), on heap buffers of
// exactly the kernels' sizes with every index asserted in bounds.  It prints what it computed --
//   pick E=<E> kind=<kind> S=<S> salt=<salt> h=<h> g=<g>
//   flow E=<E> S=<S> n=<n> salt=<salt> digest=<d>
// -- and the test recomputes every line with numpy (util/symmetry.py pick_hashes / pick_elements /
// pick_forward), so the two statements of the definition are held to each other exactly.
#include "../galvanise_zero_amd/csrc/nn/symmetry.h"

#include <cassert>
#include <cstdint>
#include <cstring>

using namespace gzsym;

// a row of 0.0 / 1.0 from a 32-bit LCG (the test restates it)
static void lcg_row(unsigned seed, int E, unsigned* bits) {
    unsigned x = seed;
    for (int i = 0; i < E; ++i) {
        x = x * 1664525u + 1013904223u;
        bits[i] = ((x >> 16) & 1u) ? 0x3F800000u : 0u;
    }
}

static void make_row(const char* kind, int E, unsigned* bits) {
    for (int i = 0; i < E; ++i) bits[i] = 0u;
    if (!strcmp(kind, "one")) for (int i = 0; i < E; ++i) bits[i] = 0x3F800000u;
    if (!strcmp(kind, "negzero")) bits[0] = 0x80000000u;          // -0.0 where "zero" holds 0.0
    if (!strcmp(kind, "nan")) bits[E - 1] = 0x7FC00123u;          // a NaN with a payload
    if (!strcmp(kind, "lcg")) lcg_row(12345u + (unsigned)E, E, bits);
}

// the hash in another order (pairs from both ends, then a 4-lane strided tree): the sum is modular
static unsigned hash_reordered(const unsigned* bits, int E) {
    unsigned lane[4] = {0, 0, 0, 0};
    for (int i = E - 1; i >= 0; --i) lane[i & 3] += pick_term(bits[i], (unsigned)i);
    return (lane[3] + lane[1]) + (lane[2] + lane[0]);
}

static void check_picks() {
    const int Es[] = {1, 3, 75, 320, 5415};
    const char* kinds[] = {"zero", "one", "negzero", "nan", "lcg"};
    const int Ss[] = {1, 2, 3, 8};
    const unsigned salts[] = {0u, 0xFFFFFFFFu};
    for (int E : Es) {
        std::vector<unsigned> bits((size_t)E);
        unsigned h_zero = 0;
        for (const char* kind : kinds) {
            make_row(kind, E, bits.data());
            const unsigned h = pick_hash(bits.data(), E);
            assert(h == hash_reordered(bits.data(), E));
            if (!strcmp(kind, "zero")) h_zero = h;
            if (!strcmp(kind, "negzero")) assert(h != h_zero);    // the hash reads bit patterns
            for (int S : Ss)
                for (unsigned salt : salts) {
                    const int g = pick_element(h, salt, S);
                    assert(g >= 0 && g < S);
                    printf("pick E=%d kind=%s S=%d salt=%u h=%u g=%d\n", E, kind, S, salt, h, g);
                }
        }
    }
    // the extremes of the multiply-shift: never S
    for (int S = 1; S <= kMaxCount; ++S) {
        unsigned lo = 0xFFFFFFFFu, hi = 0;
        for (unsigned h = 0; h < 200000u; ++h) {
            const unsigned g = (unsigned)pick_element(h * 2654435761u, 77u, S);
            lo = g < lo ? g : lo;
            hi = g > hi ? g : hi;
        }
        assert(lo == 0 && hi == (unsigned)S - 1);
    }
}

static unsigned digest(const std::vector<float>& a, unsigned d) {
    for (size_t i = 0; i < a.size(); ++i) {
        unsigned b;
        std::memcpy(&b, &a[i], 4);
        d += fmix32(b + 0x9E3779B9u * (unsigned)(i + 1));
    }
    return d;
}

// n rows through expand, a stand-in forward and the gather over `nseg` segments, exactly-sized buffers.
// Tables: element s rotates by 3 s (planes) and 2 s + r (role r's moves); the stand-in forward is
// raw_r[m] = x[(5 m + r) % E] + m and values[v] = 2 x[v % E] + v (exact in float).
static void check_flow(int E, int S, int n, unsigned salt, int nseg) {
    const int R = 2, P[2] = {7, 12}, V = 3;
    OutLayout L{};
    L.R = R;
    L.V = V;
    L.S = S;
    L.total = V + P[0] + P[1];
    L.P[0] = P[0];
    L.P[1] = P[1];
    std::vector<int> plane((size_t)S * E);
    std::vector<int> moves[2];
    for (int s = 0; s < S; ++s)
        for (int i = 0; i < E; ++i) plane[(size_t)s * E + i] = (i + 3 * s) % E;
    for (int r = 0; r < R; ++r) {
        moves[r].resize((size_t)S * P[r]);
        for (int s = 0; s < S; ++s)
            for (int m = 0; m < P[r]; ++m) moves[r][(size_t)s * P[r] + m] = s == 0 ? m : (m + 2 * s + r) % P[r];
    }
    std::vector<float> in((size_t)n * E);
    for (int r = 0; r < n; ++r) {
        std::vector<unsigned> bits((size_t)E);
        lcg_row(1000u + 31u * (unsigned)r + (unsigned)E, E, bits.data());
        std::memcpy(in.data() + (size_t)r * E, bits.data(), (size_t)E * 4);
    }
    // sym_pick_expand_kernel: one workgroup per row
    std::vector<int> picks((size_t)n, -1);
    std::vector<float> x((size_t)n * E, -1.f);
    for (int r = 0; r < n; ++r) {
        std::vector<unsigned> bits((size_t)E);
        std::memcpy(bits.data(), in.data() + (size_t)r * E, (size_t)E * 4);
        const int g = pick_element(pick_hash(bits.data(), E), salt, S);
        picks[(size_t)r] = g;
        for (int i = 0; i < E; ++i) {
            const size_t src = pick_expand_src(r, i, g, E, plane.data());
            assert(src >= (size_t)r * E && src < (size_t)(r + 1) * E);   // within the row
            x[(size_t)r * E + i] = in[src];
        }
    }
    // stand-in forward: raw outputs [n][P_r] per role, [n][V]
    std::vector<float> raw[3];
    for (int k = 0; k <= R; ++k) {
        const int width = k < R ? P[k] : V;
        raw[k].resize((size_t)n * width);
        for (int r = 0; r < n; ++r)
            for (int m = 0; m < width; ++m)
                raw[k][(size_t)r * width + m] = k < R ? x[(size_t)r * E + (5 * m + k) % E] + (float)m : 2.f * x[(size_t)r * E + m % E] + (float)m;
    }
    // sym_pick_gather_kernel into nseg separately allocated destinations of uneven sizes
    PickSegments sg{};
    sg.nseg = nseg;
    std::vector<std::vector<float>> dst((size_t)nseg * (R + 1));
    for (int k = 0, row = 0; k < nseg; ++k) {
        const int rows = k + 1 < nseg ? (n - row) / 2 : n - row;       // may be 0: an empty segment
        sg.row0[k] = row;
        for (int j = 0; j <= R; ++j) {
            dst[(size_t)k * (R + 1) + j].assign((size_t)rows * (j < R ? P[j] : V), -1.f);
            sg.out[k][j] = dst[(size_t)k * (R + 1) + j].data();
        }
        row += rows;
    }
    for (int r = 0; r < n; ++r)
        for (int j = 0; j < L.total; ++j) {
            int role, m;
            split_column(L, j, &role, &m);
            const int width = role < R ? P[role] : V;
            const int k = pick_find_segment(sg, r);
            assert(k >= 0 && k < nseg && r >= sg.row0[k] && (k + 1 == nseg || r < sg.row0[k + 1]));
            const size_t at = (size_t)(r - sg.row0[k]) * width + m;
            assert(at < dst[(size_t)k * (R + 1) + role].size());
            const size_t src = pick_gather_src(r, m, picks[(size_t)r], width, role < R ? moves[role].data() : nullptr);
            assert(src >= (size_t)r * width && src < (size_t)(r + 1) * width);
            assert(sg.out[k][role][at] == -1.f);                        // every element written once
            sg.out[k][role][at] = raw[role][src];
        }
    // against the definition, and the digest the test recomputes: roles then values, rows in order
    unsigned d = 0;
    for (int j = 0; j <= R; ++j) {
        const int width = j < R ? P[j] : V;
        std::vector<float> all;
        for (int k = 0; k < nseg; ++k) all.insert(all.end(), dst[(size_t)k * (R + 1) + j].begin(), dst[(size_t)k * (R + 1) + j].end());
        assert(all.size() == (size_t)n * width);
        for (int r = 0; r < n; ++r)
            for (int m = 0; m < width; ++m) {
                const int g = picks[(size_t)r];
                const int mm = j < R ? moves[j][(size_t)g * width + m] : m;
                assert(all[(size_t)r * width + m] == raw[j][(size_t)r * width + mm]);
            }
        d = digest(all, d);
    }
    printf("flow E=%d S=%d n=%d salt=%u digest=%u\n", E, S, n, salt, d);
}

int main() {
    check_picks();
    const int Es[] = {1, 3, 75, 320, 5415};
    const int Ss[] = {1, 2, 3, 8};
    for (int E : Es)
        for (int S : Ss) {
            check_flow(E, S, 5, 0u, 1);
            check_flow(E, S, 9, 0xFFFFFFFFu, 4);
        }
    check_flow(75, 8, 40, 12345u, kMaxPickSegments);
    printf("symmetry pick host check passed\n");
    return 0;
}
