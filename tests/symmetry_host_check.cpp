// Stand-alone CPU check of csrc/nn/symmetry.h (built with -fsanitize=address,undefined by
// tests/test_symmetry_tables.py): the table validation's refusals, and both kernels' index arithmetic
// -- sym_expand_kernel's expand_src and sym_reduce_kernel's split_column / reduce_one -- walked over
// small tables on heap buffers of exactly the kernels' sizes, every index asserted in bounds and the
// results compared with a direct restatement of the ensemble.
#include "../galvanise_zero_amd/csrc/nn/symmetry.h"

#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <random>

using namespace gzsym;

static std::vector<int> random_perms(std::mt19937& rng, int S, int len, bool identity_first) {
    std::vector<int> t((size_t)S * len);
    for (int s = 0; s < S; ++s) {
        int* p = t.data() + (size_t)s * len;
        for (int i = 0; i < len; ++i) p[i] = i;
        if (s > 0 || !identity_first)
            for (int i = len - 1; i > 0; --i) std::swap(p[i], p[rng() % (unsigned)(i + 1)]);
    }
    return t;
}

static void expect_refusal(const std::string& got, const char* want) {
    if (got.find("symmetry: ") != 0 || got.find(want) == std::string::npos) {
        printf("FAIL: expected a refusal containing '%s', got '%s'\n", want, got.c_str());
        exit(1);
    }
    printf("refusal ok: %s\n", got.c_str());
}

static void check_validation() {
    std::mt19937 rng(7);
    const int E = 12, P[2] = {5, 7};
    for (int S = 1; S <= kMaxCount; ++S) {
        std::vector<int> plane = random_perms(rng, S, E, true);
        std::vector<int> m0 = random_perms(rng, S, P[0], true), m1 = random_perms(rng, S, P[1], true);
        const int* moves[2] = {m0.data(), m1.data()};
        assert(validate_tables(S, E, plane.data(), 2, P, moves).empty());
        if (S < 2) continue;
        std::vector<int> bad = plane;
        bad[(size_t)(S - 1) * E + 3] = bad[(size_t)(S - 1) * E + 4];   // a duplicate
        char want[64];
        snprintf(want, sizeof want, "plane table of element %d", S - 1);
        expect_refusal(validate_tables(S, E, bad.data(), 2, P, moves), want);
        bad = plane;
        bad[(size_t)(S - 1) * E] = E;                                    // out of range
        expect_refusal(validate_tables(S, E, bad.data(), 2, P, moves), want);
        bad[(size_t)(S - 1) * E] = -1;
        expect_refusal(validate_tables(S, E, bad.data(), 2, P, moves), want);
        std::vector<int> badm = m1;
        badm[(size_t)(S - 1) * P[1] + 6] = badm[(size_t)(S - 1) * P[1]];
        const int* moves2[2] = {m0.data(), badm.data()};
        snprintf(want, sizeof want, "move table of element %d, role 1", S - 1);
        expect_refusal(validate_tables(S, E, plane.data(), 2, P, moves2), want);
    }
    std::vector<int> plane = random_perms(rng, 9, E, true), m0 = random_perms(rng, 9, P[0], true);
    const int* moves[1] = {m0.data()};
    expect_refusal(validate_tables(0, E, plane.data(), 1, P, moves), "count 0 outside 1..8");
    expect_refusal(validate_tables(9, E, plane.data(), 1, P, moves), "count 9 outside 1..8");
    expect_refusal(validate_tables(2, E, nullptr, 1, P, moves), "null table");
    expect_refusal(validate_tables(2, E, plane.data(), 5, P, moves), "roles 5");
}

// one chunk of n rows through the kernels' arithmetic, exactly-sized buffers
static void check_chunk(std::mt19937& rng, int S, int n, int E, int R, const int* P, int V) {
    std::vector<int> plane = random_perms(rng, S, E, false);
    std::vector<std::vector<int>> moves(R);
    OutLayout L{};
    L.R = R;
    L.V = V;
    L.S = S;
    L.total = V;
    for (int r = 0; r < R; ++r) {
        moves[r] = random_perms(rng, S, P[r], false);
        L.P[r] = P[r];
        L.total += P[r];
    }
    std::uniform_real_distribution<float> u(0.f, 1.f);
    std::vector<float> in((size_t)n * E);
    for (float& f : in) f = u(rng);

    // sym_expand_kernel: one thread per output element
    const size_t total = (size_t)S * n * E;
    std::vector<float> x(total);
    for (size_t o = 0; o < total; ++o) {
        const size_t src = expand_src(o, n, E, plane.data());
        assert(src < in.size());
        x[o] = in[src];
    }
    for (int s = 0; s < S; ++s)
        for (int r = 0; r < n; ++r)
            for (int i = 0; i < E; ++i)
                assert(x[(expanded_row(s, r, n)) * E + i] == in[(size_t)r * E + plane[(size_t)s * E + i]]);

    // raw outputs of the S * n rows (stand-ins), then sym_reduce_kernel: one thread per (row, column)
    std::vector<std::vector<float>> raw(R + 1), out(R + 1);
    for (int k = 0; k <= R; ++k) {
        const int width = k < R ? P[k] : V;
        raw[k].resize((size_t)S * n * width);
        out[k].assign((size_t)n * width, -1.f);
        for (float& f : raw[k]) f = u(rng);
    }
    for (int r = 0; r < n; ++r)
        for (int j = 0; j < L.total; ++j) {
            int role, m;
            split_column(L, j, &role, &m);
            assert(role >= 0 && role <= R);
            const int width = role < R ? P[role] : V;
            assert(m >= 0 && m < width);
            const int* src = role < R ? moves[role].data() : nullptr;
            for (int s = 0; s < S; ++s) {   // the reads reduce_one makes
                const size_t at = expanded_row(s, r, n) * (size_t)width + (size_t)(src ? src[(size_t)s * width + m] : m);
                assert(at < raw[role].size());
            }
            float& o = out[role][(size_t)r * width + m];
            assert(o == -1.f);              // every element written once
            o = reduce_one(raw[role].data(), src, S, n, r, width, m);
        }
    // restatement: sum in element order, exact scale for powers of two
    for (int k = 0; k <= R; ++k) {
        const int width = k < R ? P[k] : V;
        for (int r = 0; r < n; ++r)
            for (int m = 0; m < width; ++m) {
                volatile float acc = 0.f;
                for (int s = 0; s < S; ++s) {
                    const int mm = k < R ? moves[k][(size_t)s * width + m] : m;
                    const float term = raw[k][((size_t)s * n + r) * width + mm];
                    acc = s == 0 ? term : acc + term;
                }
                const float want = (S & (S - 1)) == 0 ? acc * (1.0f / (float)S) : acc / (float)S;
                const float got = out[k][(size_t)r * width + m];
                if (std::memcmp(&want, &got, 4) != 0) {
                    printf("FAIL: S=%d n=%d role %d row %d m %d: %a vs %a\n", S, n, k, r, m, got, want);
                    exit(1);
                }
            }
    }
    printf("chunk ok: S=%d n=%d E=%d R=%d P0=%d V=%d\n", S, n, E, R, P[0], V);
}

int main() {
    check_validation();
    std::mt19937 rng(11);
    const int P1[1] = {9}, P2[2] = {13, 17}, P4[4] = {3, 1, 5, 2};
    for (int S = 1; S <= kMaxCount; ++S) {
        check_chunk(rng, S, 1, 20, 2, P2, 2);
        check_chunk(rng, S, 5, 45, 1, P1, 3);
        check_chunk(rng, S, 3, 7, 4, P4, 2);
    }
    // chunking: rows per chunk for every S, the environment's lower bound honoured, never raised
    for (int S = 1; S <= kMaxCount; ++S) {
        assert(chunk_rows(S, 0) * S <= kMaxExpandedRows && chunk_rows(S, 0) >= 1);
        assert(chunk_rows(S, 2) == 2);
        assert(chunk_rows(S, 1 << 20) == chunk_rows(S, 0));
        assert(chunk_rows(S, -3) == chunk_rows(S, 0));
    }
    printf("symmetry host check passed\n");
    return 0;
}
