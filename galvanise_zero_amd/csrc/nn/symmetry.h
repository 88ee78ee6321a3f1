// Symmetry ensemble (include/gzero_nn.h gz_symmetry): a forward averaged over the S <= 8 elements of
// a board's symmetry group.  With the caller's tables plane_src[s][E] and move_src[s][r][P_r], row r
// of a call computes
//
//   X_s[i]  = X_r[plane_src[s][i]]                               sym_expand_kernel
//   p_s, v_s = the net's ordinary forward of X_s                 gz_net_forward_device, S * rows rows
//   out[m]  = (p_0[move_src[0][m]] + p_1[move_src[1][m]] + ...) * (1 / S)      sym_reduce_kernel
//
// in fp32 and in that order: acc starts as element 0's term, elements 1 .. S - 1 are added in
// ascending order, and the scale is the exact product by 1 / S when S is a power of two and the
// division acc / S otherwise.  Values are summed alike, without a permutation.  The forward is
// batch-invariant, so a row's result depends on that row's planes and the tables alone.
//
// Scratch bound: one inner forward runs at most kMaxExpandedRows (2,048) expanded rows, so a call
// goes through in chunks of chunk_rows(S) = 2,048 / S rows (256 rows for S = 8) and the object's
// scratch holds at most 2,048 x (E + sum P_r + V) floats of expanded planes and raw outputs, plus
// chunk_rows x (E + sum P_r + V) of staging for the host entry point -- 67 MB for amazons_10x10
// (E = 1,200, P = 3,041 + 3,041), the largest game here.  GZ_SYM_CHUNK_ROWS in the environment lowers
// the rows per chunk (tests), never raises them.
//
// The index arithmetic of both kernels and the table validation are plain / __host__ __device__
// functions here, so that a CPU program can run them (tests/symmetry_host_check.cpp).
//
// Below the ensemble: one symmetry per row, picked from a hash of the row's own planes
// (gz_net_forward_sym_pick, gz_runner_set_symmetry) -- the definition, likewise as functions a CPU
// program runs (tests/symmetry_pick_host_check.cpp).
//
// Below the pick: the canonical orientation (gz_net_forward_sym_canon, gz_runner_set_canonical) -- the
// element is the one that maps the row to its symmetry class's canonical image, so symmetric
// positions share one forward and one cache entry (tests/symmetry_canon_host_check.cpp).
#pragma once

#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/gzero_nn.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GZSYM_HD __host__ __device__
#else
#define GZSYM_HD
#endif

namespace gzsym {

constexpr int kMaxCount = 8;
constexpr int kMaxExpandedRows = 2048;

// Expanded rows are element-major: element s of row r of a chunk of n rows is row s * n + r.
GZSYM_HD inline size_t expanded_row(int s, int r, int n) { return (size_t)s * (size_t)n + (size_t)r; }

// sym_expand_kernel, output element o of [S * n][E]: where it reads in the chunk's planes [n][E].
GZSYM_HD inline size_t expand_src(size_t o, int n, int E, const int* plane_src) {
    const size_t row = o / (size_t)E;
    const int i = (int)(o - row * (size_t)E);
    const int s = (int)(row / (size_t)n);
    const int r = (int)(row - (size_t)s * (size_t)n);
    return (size_t)r * (size_t)E + (size_t)plane_src[(size_t)s * E + i];
}

// The outputs of one row, all roles then the values, as one index space [0, sum P_r + V).
struct OutLayout {
    int R, V, S;
    int P[GZ_MAX_ROLES];
    int total;                                   // sum P_r + V
};

// Column j of a row: role (R for the values) and index within it.
GZSYM_HD inline void split_column(const OutLayout& L, int j, int* role, int* m) {
    int r = 0;
    while (r < L.R && j >= L.P[r]) { j -= L.P[r]; ++r; }
    *role = r;
    *m = j;
}

// sym_reduce_kernel, one output element: `raw` is the role's (or the values') raw outputs
// [S * n][width], `src` the role's move table [S][width] (nullptr for the values).
GZSYM_HD inline float reduce_one(const float* raw, const int* src, int S, int n, int r, int width, int m) {
    float acc = raw[expanded_row(0, r, n) * (size_t)width + (size_t)(src ? src[m] : m)];
    for (int s = 1; s < S; ++s)
        acc += raw[expanded_row(s, r, n) * (size_t)width + (size_t)(src ? src[(size_t)s * width + m] : m)];
    if ((S & (S - 1)) == 0) return acc * (1.0f / (float)S);
    return acc / (float)S;
}

// Rows per chunk for S elements; env_rows > 0 (GZ_SYM_CHUNK_ROWS) lowers it.
inline int chunk_rows(int S, int env_rows) {
    int c = kMaxExpandedRows / (S < 1 ? 1 : S);
    if (env_rows > 0 && env_rows < c) c = env_rows;
    return c < 1 ? 1 : c;
}

// ---- one symmetry per row, picked from the row's own planes (gz_net_forward_sym_pick) -------------
// For a row of E plane elements with 32-bit patterns b_i as stored (-0.0 is not 0.0, a NaN is its
// bits), S table elements and a 32-bit salt, all in wrapping uint32 arithmetic:
//
//   h = sum over i in [0, E) of fmix(b_i + 0x9E3779B9 * (i + 1))         pick_term, any order
//   g = (uint64(fmix(h ^ salt)) * S) >> 32                                pick_element, in [0, S)
//   X'[i] = X[plane_src[g][i]]                                            sym_pick_expand_kernel
//   p', v' = the net's ordinary forward of X'
//   out_r[m] = p'_r[move_src[g][r][m]],  values = v'                      sym_pick_gather_kernel
//
// The sum is modular, so every reduction tree gives the same h: the kernel's wave shuffles and the
// loop below agree exactly.  No floating-point operation is added, so a picked row is bit for bit the
// plain forward of the permuted planes read through the move table.  g is a function of the row's
// planes, S and the salt alone: the same position gets the same element in any batch, slot or entry
// point -- which a host RNG draw per leaf would not give.
GZSYM_HD inline unsigned fmix32(unsigned x) {
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}

// element i's term of the row hash
GZSYM_HD inline unsigned pick_term(unsigned bits, unsigned i) { return fmix32(bits + 0x9E3779B9u * (i + 1u)); }

GZSYM_HD inline int pick_element(unsigned h, unsigned salt, int S) {
    return (int)(((unsigned long long)fmix32(h ^ salt) * (unsigned long long)S) >> 32);
}

// the row hash, serially (the CPU statement of what sym_pick_expand_kernel reduces in parallel)
inline unsigned pick_hash(const unsigned* bits, int E) {
    unsigned h = 0;
    for (int i = 0; i < E; ++i) h += pick_term(bits[i], (unsigned)i);
    return h;
}

// sym_pick_expand_kernel, element i of row r picked as g: where it reads in the planes [n][E]
GZSYM_HD inline size_t pick_expand_src(int r, int i, int g, int E, const int* plane_src) {
    return (size_t)r * (size_t)E + (size_t)plane_src[(size_t)g * E + i];
}

// sym_pick_gather_kernel, column m of row r of a role `width` wide: where it reads in the role's raw
// outputs [n][width]; src is the role's move table [S][width], nullptr for the values
GZSYM_HD inline size_t pick_gather_src(int r, int m, int g, int width, const int* src) {
    return (size_t)r * (size_t)width + (size_t)(src ? src[(size_t)g * width + m] : m);
}

// Destinations of a gather launch: segment k holds rows [row0[k], row0[k + 1]) of the launch, written
// to out[k][role] + (row - row0[k]) * width (role R: the values).  GZ_MAX_SEGMENTS segments at most.
constexpr int kMaxPickSegments = 32;
struct PickSegments {
    int nseg;
    int row0[kMaxPickSegments];
    float* out[kMaxPickSegments][GZ_MAX_ROLES + 1];
};

GZSYM_HD inline int pick_find_segment(const PickSegments& sg, int row) {
    int s = 0;
    while (s + 1 < sg.nseg && row >= sg.row0[s + 1]) ++s;
    return s;
}

}  // namespace gzsym

// The evaluation cache's row tag (eval_cache.h states the cache; these four are here because the
// canonical orientation below ranks a row's images by that tag).
namespace gzcache {

GZSYM_HD inline unsigned mix32b(unsigned x) {
    x ^= x >> 15;
    x *= 0x2c1b3c6du;
    x ^= x >> 12;
    x *= 0x297a2d39u;
    x ^= x >> 15;
    return x;
}

// element i's term of the second row hash (the first is gzsym::pick_term)
GZSYM_HD inline unsigned hash2_term(unsigned bits, unsigned i) { return mix32b(bits + 0x85EBCA77u * (i + 1u)); }

GZSYM_HD inline unsigned long long make_tag(unsigned h1, unsigned h2) {
    return ((unsigned long long)h2 << 32) | (unsigned long long)h1;
}

GZSYM_HD inline unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

}  // namespace gzcache

namespace gzsym {

// ---- canonical orientation: every member of a symmetry class evaluated as the same image -----------
// (gz_net_forward_sym_canon, gz_runner_set_canonical).  For a row X of E plane words as 32-bit patterns
// (pick_term's reading), tables of S <= 8 elements and a 32-bit salt:
//
//   X_s[i] = X[plane_src[s][i]]                                  image s, s in [0, S)
//   t_s    = make_tag(pick_hash(X_s), hash2(X_s))                the cache's 64-bit row tag of image s
//   k_s    = mix64(t_s ^ uint64(salt))                           a bijection of the tag: another salt,
//                                                                another representative
//   g      = the s with the smallest (k_s, s)                    ties, equal images included: lowest s
//   X'     = X_g;  p', v' = the net's ordinary forward of X'     or, with a cache, the cached forward
//   out_r[m] = p'_r[move_src[r][g][m]];  values = v'             sym_pick_gather_kernel, unchanged
//
// Both hashes are modular sums, so sym_canon_expand_kernel's reduction tree and the loops below agree.
//
// 1. No floating-point operation is added.  g depends on the row, the tables and the salt alone: a
//    row is bit for bit the plain forward of X_g read through move_src[g], in any batch, chunk, entry
//    point or replay.  S = 1 with the identity is gz_net_forward.  Tables that are no group are served;
//    they get this property and nothing more.
// 2. Symmetric positions share one image.  Where the tables are closed under composition (every
//    game's are), the images of Y = X_t are the images of X, so both rows get the same X' -- through a
//    cache the second one hits -- and, if X's S images are all distinct,
//    out_X[r][m] == out_Y[r][move_src[r][t][m]] exactly for every t and m (by
//    move_src[c] = move_src[b][move_src[a]] for c = "a then b").  The ensemble gives that to 1e-6 only.
// 3. A position that is its own image (X_s == X_t, s != t) is evaluated correctly, under the lowest
//    such s; property 2's equality is not promised for it (a net's output on a symmetric board need
//    not be symmetric).  A tag collision between different images (2^-64 a pair) can cost sharing,
//    never correctness: the cache's compare of all plane words decides alone.
GZSYM_HD inline unsigned long long canon_key(unsigned long long tag, unsigned salt) {
    return gzcache::mix64(tag ^ (unsigned long long)salt);
}

// g from the S images' hash totals (h1[s], h2[s]); *tag = t_g
GZSYM_HD inline int canon_pick(const unsigned* h1, const unsigned* h2, int S, unsigned salt, unsigned long long* tag) {
    int g = 0;
    unsigned long long best_tag = gzcache::make_tag(h1[0], h2[0]);
    unsigned long long best = canon_key(best_tag, salt);
    for (int s = 1; s < S; ++s) {
        const unsigned long long t = gzcache::make_tag(h1[s], h2[s]), k = canon_key(t, salt);
        if (k < best) { best = k; best_tag = t; g = s; }
    }
    *tag = best_tag;
    return g;
}

// the definition, serially: g of one row; *tag (may be null) = t_g
inline int canon_element(const unsigned* bits, int E, int S, const int* plane_src, unsigned salt, unsigned long long* tag) {
    unsigned h1[kMaxCount] = {}, h2[kMaxCount] = {};
    for (int s = 0; s < S; ++s)
        for (int i = 0; i < E; ++i) {
            const unsigned b = bits[plane_src[(size_t)s * E + i]];
            h1[s] += pick_term(b, (unsigned)i);
            h2[s] += gzcache::hash2_term(b, (unsigned)i);
        }
    unsigned long long t = 0;
    const int g = canon_pick(h1, h2, S, salt, &t);
    if (tag) *tag = t;
    return g;
}

// sym_canon_expand_kernel keeps a row in LDS when it has at most this many words (32 KiB: five
// workgroups a CU; the largest game here has 5,415); a longer row is gathered from global memory
constexpr int kCanonLdsWords = 8192;

// true when t[0 .. len) holds every value of 0 .. len - 1 once; else *bad = the first offending entry
inline bool is_permutation(const int* t, int len, int* bad) {
    std::vector<char> seen((size_t)len, 0);
    for (int i = 0; i < len; ++i) {
        if (t[i] < 0 || t[i] >= len || seen[(size_t)t[i]]) { *bad = i; return false; }
        seen[(size_t)t[i]] = 1;
    }
    return true;
}

// Everything gz_symmetry_create checks, before any device call.  Returns "" or the refusal.
inline std::string validate_tables(int count, int plane_elems, const int* plane_src, int roles,
                                   const int* policy_sizes, const int* const* move_src) {
    char b[200];
    if (count < 1 || count > kMaxCount) {
        snprintf(b, sizeof b, "symmetry: count %d outside 1..%d", count, kMaxCount);
        return b;
    }
    if (plane_elems < 1 || roles < 1 || roles > GZ_MAX_ROLES) {
        snprintf(b, sizeof b, "symmetry: plane_elems %d or roles %d out of range (roles 1..%d)", plane_elems, roles, GZ_MAX_ROLES);
        return b;
    }
    if (!plane_src || !policy_sizes || !move_src) return "symmetry: null table";
    for (int r = 0; r < roles; ++r) {
        if (policy_sizes[r] < 1) {
            snprintf(b, sizeof b, "symmetry: policy size %d of role %d out of range", policy_sizes[r], r);
            return b;
        }
        if (!move_src[r]) return "symmetry: null table";
    }
    int bad = 0;
    for (int s = 0; s < count; ++s) {
        if (!is_permutation(plane_src + (size_t)s * plane_elems, plane_elems, &bad)) {
            snprintf(b, sizeof b, "symmetry: plane table of element %d is not a permutation of 0..%d (entry %d = %d)", s,
                     plane_elems - 1, bad, plane_src[(size_t)s * plane_elems + bad]);
            return b;
        }
        for (int r = 0; r < roles; ++r)
            if (!is_permutation(move_src[r] + (size_t)s * policy_sizes[r], policy_sizes[r], &bad)) {
                snprintf(b, sizeof b, "symmetry: move table of element %d, role %d is not a permutation of 0..%d (entry %d = %d)",
                         s, r, policy_sizes[r] - 1, bad, move_src[r][(size_t)s * policy_sizes[r] + bad]);
                return b;
            }
    }
    return "";
}

// What the ensemble needs to know of a net (gz_nn.hip defines both; gz_net is private to it).
struct NetView {
    int device;
    int plane_elems;                             // C * H * W
    int roles, num_values;
    int policy[GZ_MAX_ROLES];
    int logits;                                  // gz_net_set_output_logits mode, read under the net's lock
    void* host_stream;                           // the stream of the net's synchronous host-buffer forward
};
void net_view(gz_net* net, NetView* out);
int set_error(const std::string& msg);           // gz_nn_last_error's message; returns -1

#if defined(__HIPCC__)
// The pick path's pieces for a caller that owns its buffers and issues the net's forward itself (the
// self-play runner; symmetry.hip defines them and uses them for its own entry points).
// pick_check: the refusals of a pick forward, no device call.  pick_prepare: tables to the device
// (once).  pick_expand_launch: rows [0, n) of d_in [n][E] hashed, picks[r] = g and x[r] = the row
// permuted by element g (x == nullptr: the picks alone).  pick_gather_launch: raw[role] [n][P_r] and
// raw[R] [n][V] read through move_src[picks[r]] into the segments' destinations.  One launch each.
int pick_check(gz_net* net, gz_symmetry* s, NetView* v);
int pick_prepare(gz_symmetry* s, const NetView& v);
int pick_expand_launch(gz_symmetry* s, hipStream_t stream, unsigned salt, const float* d_in, int n, int* d_picks, float* d_x);
int pick_gather_launch(gz_symmetry* s, hipStream_t stream, const int* d_picks, int n, const float* const* d_raw,
                       const PickSegments& segs);
// canon_expand_launch: pick_expand_launch with the canonical g (sym_canon_expand_kernel); d_tags (may
// be null) receives each row's t_g.  The gather is the pick's.
int canon_expand_launch(gz_symmetry* s, hipStream_t stream, unsigned salt, const float* d_in, int n, int* d_picks,
                        unsigned long long* d_tags, float* d_x);
#endif

}  // namespace gzsym
