// Evaluation cache (include/gzero_nn.h gz_eval_cache): a direct-mapped table in HBM that returns the
// stored outputs of a row evaluated before.  Every forward mode computes a row's outputs from that
// row alone, so the stored bits are the bits the forward would write again: the cache is exact.
//
// Key.  A row's E = C * H * W plane words b_i as stored, read as 32-bit patterns (-0.0 is not 0.0, a
// NaN is its bits -- gzsym::pick_term's reading).  In wrapping uint32 arithmetic
//
//   h1 = sum over i of fmix32(b_i + 0x9E3779B9 * (i + 1))        gzsym::pick_hash as it stands
//   h2 = sum over i of mix32b(b_i + 0x85EBCA77 * (i + 1))        another mixer, another stride
//   tag = h2 << 32 | h1                                          64 bits
//   slot = mix64(tag) % N                                        any N >= 1
//
// Both sums are modular: any reduction tree gives the same value, so the kernel's wave shuffles and
// the serial loops below agree exactly.
//
// Table.  N entries of entry_words(E, T) 32-bit words (T = sum P_r + V): {tag, epoch} (two 64-bit
// words), the E plane words, the T output floats, each part padded to 16 bytes.  An entry is valid
// when its epoch is the cache's current one; a flush is ++epoch.  The table starts zeroed and the
// current epoch starts at 1, so epoch 0 is never current.
//
// A hit needs the epoch, the tag (the low tag_bits of it: GZ_EVAL_CACHE_TAG_BITS lowers 64, for
// tests) and all E plane words equal.  The tag is a filter; the full compare is what makes the cache
// exact.
//
// Insertion.  A call goes through in chunks of at most kMaxChunkRows rows
// (GZ_EVAL_CACHE_CHUNK_ROWS lowers it).  Every chunk has a sequence number of its own, one more than
// the chunk before it (of this call or an earlier one).  All rows of a chunk are probed before any
// is inserted.  A missed row claims its slot by a 64-bit atomicMax of claim_word(seq, row) -- seq in
// the high 48 bits, ~row (the row's index in the chunk) in the low 16: a newer chunk beats an older
// one, and within a chunk the lowest row wins.  After the forward of the misses, only the row that
// holds its slot's claim writes the entry (planes, outputs, then the header): no entry is written by
// two rows.  Rows of one chunk with equal planes all miss and all go through the forward; the lowest
// inserts.  48 bits of sequence last 890 years at 10^4 chunks a second: no wrap.
//
// So which rows hit, and which entries exist after any sequence of calls, is a function of that
// sequence, N and the chunk size alone (the tag bits filter before a compare that decides alone).
// Model states it serially; galvanise_zero_amd/util/evalcache.py states it again in numpy, and
// tests/eval_cache_host_check.cpp runs this one.
#pragma once

#include <cstdint>
#include <map>
#include <vector>

#include "symmetry.h"

namespace gzcache {

constexpr int kMaxChunkRows = 2048;              // < 1 << 16: a row's index fits the claim word
constexpr long long kMaxTableBytes = 16ll << 30; // gz_eval_cache_create refuses a larger table

// mix32b, hash2_term, make_tag and mix64 are in symmetry.h (namespace gzcache): the canonical
// orientation there ranks a row's images by this tag.

GZSYM_HD inline unsigned long long slot_of(unsigned long long tag, unsigned long long N) { return mix64(tag) % N; }

// the tag bits a probe compares: the low `bits` of the 64
GZSYM_HD inline unsigned long long tag_mask(int bits) {
    return bits >= 64 ? ~0ull : bits <= 0 ? 0ull : ((1ull << bits) - 1ull);
}

GZSYM_HD inline unsigned long long claim_word(unsigned long long seq, int row) {
    return (seq << 16) | (unsigned long long)(~(unsigned)row & 0xFFFFu);
}

// an entry in 32-bit words: header (4), planes and outputs, each padded to a multiple of 4 words
GZSYM_HD inline size_t entry_plane_off() { return 4; }
GZSYM_HD inline size_t entry_out_off(int E) { return 4 + (((size_t)E + 3) & ~(size_t)3); }
GZSYM_HD inline size_t entry_words(int E, int T) { return entry_out_off(E) + (((size_t)T + 3) & ~(size_t)3); }

// the second row hash, serially
inline unsigned hash2(const unsigned* bits, int E) {
    unsigned h = 0;
    for (int i = 0; i < E; ++i) h += hash2_term(bits[i], (unsigned)i);
    return h;
}

inline unsigned long long row_tag(const unsigned* bits, int E) { return make_tag(gzsym::pick_hash(bits, E), hash2(bits, E)); }

inline int chunk_rows(int env_rows) {
    int c = kMaxChunkRows;
    if (env_rows > 0 && env_rows < c) c = env_rows;
    return c;
}

inline int tag_bits(int env_bits, bool env_set) {
    if (!env_set || env_bits > 64) return 64;
    return env_bits < 0 ? 0 : env_bits;
}

// The cache as a serial program: the same hits and the same table as the kernels, call by call.
struct Model {
    struct Entry {
        unsigned long long tag = 0, epoch = 0;
        std::vector<unsigned> planes;
    };
    unsigned long long N;
    int E, bits, chunk;
    unsigned long long epoch = 1, seq = 0;
    std::map<unsigned long long, Entry> table;   // slot -> entry (an absent slot is a zeroed one)
    std::map<unsigned long long, unsigned long long> claim;
    long hits = 0, forward_rows = 0, inserts = 0, replaced = 0, flushes = 0;

    Model(unsigned long long entries, int plane_elems, int tag_bits_, int chunk_rows_)
        : N(entries), E(plane_elems), bits(tag_bits_), chunk(chunk_rows(chunk_rows_)) {}

    void flush() { ++epoch; ++flushes; }

    bool probe_row(const unsigned* b) const {
        const unsigned long long tag = row_tag(b, E);
        auto it = table.find(slot_of(tag, N));
        if (it == table.end()) return false;
        const Entry& e = it->second;
        if (e.epoch != epoch || ((e.tag ^ tag) & tag_mask(bits))) return false;
        for (int i = 0; i < E; ++i)
            if (e.planes[(size_t)i] != b[i]) return false;
        return true;
    }

    // rows [n][E]; returns each row's hit flag
    std::vector<int> call(const unsigned* X, int n) {
        std::vector<int> hit((size_t)n, 0);
        for (int r0 = 0; r0 < n; r0 += chunk) {
            const int c = n - r0 < chunk ? n - r0 : chunk;
            ++seq;
            for (int r = 0; r < c; ++r) {              // cache_probe_kernel: all rows before any insert
                const unsigned* b = X + (size_t)(r0 + r) * E;
                hit[(size_t)(r0 + r)] = probe_row(b) ? 1 : 0;
                if (hit[(size_t)(r0 + r)]) { ++hits; continue; }
                ++forward_rows;
                unsigned long long& cw = claim[slot_of(row_tag(b, E), N)];
                const unsigned long long mine = claim_word(seq, r);
                if (mine > cw) cw = mine;
            }
            for (int r = 0; r < c; ++r) {              // cache_fill_kernel: the claim's holder writes
                if (hit[(size_t)(r0 + r)]) continue;
                const unsigned* b = X + (size_t)(r0 + r) * E;
                const unsigned long long tag = row_tag(b, E), slot = slot_of(tag, N);
                if (claim[slot] != claim_word(seq, r)) continue;
                Entry& e = table[slot];
                ++inserts;
                if (e.epoch == epoch) ++replaced;
                e.tag = tag;
                e.epoch = epoch;
                e.planes.assign(b, b + E);
            }
        }
        return hit;
    }

    // the valid entries as one number: sum of mix64(tag ^ mix64(slot + 1)), wrapping
    unsigned long long digest() const {
        unsigned long long d = 0;
        for (const auto& kv : table)
            if (kv.second.epoch == epoch) d += mix64(kv.second.tag ^ mix64(kv.first + 1));
        return d;
    }
};

// What eval_cache.hip needs of a net beyond gzsym::NetView (gz_nn.hip defines both).  net_epoch: the
// net's weight generation, bumped by every installed image and every change of the output-logits
// mode.  forward_segments_epoch: gz_net_forward_segments, and the generation that launch ran under.
unsigned long long net_epoch(gz_net* net);
int forward_segments_epoch(gz_net* net, void* stream, const gz_segment* segs, int nseg, unsigned long long* epoch);

#if defined(__HIPCC__)
// The cache for a caller that owns its buffers and its stream (the self-play runner; eval_cache.hip
// defines them).  runner_check: the refusals of a call, no device call.  cached_launch: rows [0, n) of
// d_planes [n][E] through the cache on `stream`, row i's outputs written where `segs` says (rows of
// the launch; the destinations may be device or pinned host memory); blocks once per chunk for the
// count of misses and calls `idle` (may be null) while it waits.
int runner_check(gz_net* net, gz_eval_cache* cache);
int cached_launch(gz_net* net, gz_eval_cache* cache, hipStream_t stream, const float* d_planes, int n,
                  const gzsym::PickSegments& segs, void (*idle)(void*), void* idle_arg);
#endif

}  // namespace gzcache
