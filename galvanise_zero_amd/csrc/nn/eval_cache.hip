// The evaluation cache's three kernels and entry points (eval_cache.h states the definition; the
// net's own forward runs between compact and fill, unchanged, on the rows that missed).
#include "eval_cache.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>

using namespace gzcache;
using gzsym::NetView;
using gzsym::OutLayout;
using gzsym::PickSegments;
using gzsym::set_error;

typedef unsigned long long u64;

#define CACHECHK(x)                                                                                  \
    do {                                                                                             \
        hipError_t e_ = (x);                                                                         \
        if (e_ != hipSuccess) return set_error(std::string("eval cache: " #x ": ") + hipGetErrorString(e_)); \
    } while (0)

struct gz_eval_cache {
    gz_net* net = nullptr;
    int device = 0;
    u64 N = 0;
    int E = 0, T = 0;
    OutLayout L{};
    size_t stride = 0;                           // 32-bit words per entry
    int bits = 64, chunk = kMaxChunkRows;
    u64 epoch = 1, seq = 0;                      // the table's epoch; the last chunk's sequence number
    u64 net_epoch = 0;                           // the net's weight generation the entries belong to
    unsigned* d_table = nullptr;                 // [N][stride]
    u64* d_claim = nullptr;                      // [N]
    u64* d_counters = nullptr;                   // inserts, replaced
    // scratch of one chunk
    int* d_flags = nullptr;                      // [chunk] 1: the row missed
    int* d_list = nullptr;                       // [chunk] the rows that missed, ascending
    u64* d_slot = nullptr;                       // [chunk] a missed row's slot
    u64* d_tag = nullptr;                        // [chunk] and tag
    int* d_count = nullptr;
    float* d_gather = nullptr;                   // [chunk][E] planes of the rows that missed
    float* d_raw = nullptr;                      // [chunk][T] their raw outputs, role by role
    float* d_io = nullptr;                       // [chunk][E + T] the host entry points' staging
    int* h_count = nullptr;                      // pinned
    hipEvent_t ev = nullptr, ev_count = nullptr; // the end of the last call; the count's arrival
    hipStream_t stream = nullptr;                // gz_eval_cache_probe's
    std::mutex mu;
    long calls = 0, rows = 0, hits = 0, forward_rows = 0, flushes = 0;
};

struct ProbeArgs {
    const unsigned* in;                          // [n][E]
    int n, E, T, side;                           // side 0: the flags alone (no claim, no copy)
    int base;                                    // the chunk's first row in the call (the segments count from there)
    const unsigned* table;
    u64* claim;
    u64 N, epoch, mask, seq;
    size_t stride;
    int* flags;
    u64* slot;
    u64* tag;
    OutLayout L;
    PickSegments sg;
};

struct FillArgs {
    int nmiss, E, T, base;
    unsigned* table;
    const u64* claim;
    u64 epoch, seq;
    size_t stride;
    const int* list;
    const u64* slot;
    const u64* tag;
    const unsigned* gather;                      // [nmiss][E]
    const float* raw[GZ_MAX_ROLES + 1];          // [nmiss][P_r] per role; at index R the values [nmiss][V]
    u64* counters;
    OutLayout L;
    PickSegments sg;
};

__device__ inline unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

// dst[0 .. E) = src[0 .. E) by one wave: 16-byte accesses where both rows are 16-byte aligned
__device__ inline void wave_copy(unsigned* dst, const unsigned* src, int E, int lane) {
    int done = 0;
    if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0) {
        const int n4 = E >> 2;
        for (int i4 = lane; i4 < n4; i4 += 64) ((uint4*)dst)[i4] = ((const uint4*)src)[i4];
        done = n4 << 2;
    }
    for (int i = done + lane; i < E; i += 64) dst[i] = src[i];
}

// One wave per row: the row's two hashes (16-byte loads where the row is 16-byte aligned, a scalar
// loop otherwise and for the tail), the slot's header, on a filter match the compare of all E words;
// a hit copies the stored outputs to the row's destinations, a miss flags the row and claims the slot.
__global__ void __launch_bounds__(256) cache_probe_kernel(ProbeArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.n) return;
    const unsigned* b = a.in + (size_t)row * a.E;
    const bool aligned = ((uintptr_t)b & 15) == 0;
    unsigned h1 = 0, h2 = 0;
    int done = 0;
    if (aligned) {
        const int n4 = a.E >> 2;
        for (int i4 = lane; i4 < n4; i4 += 64) {
            const uint4 v = ((const uint4*)b)[i4];
            const unsigned i = 4u * (unsigned)i4;
            h1 += gzsym::pick_term(v.x, i) + gzsym::pick_term(v.y, i + 1) + gzsym::pick_term(v.z, i + 2) + gzsym::pick_term(v.w, i + 3);
            h2 += hash2_term(v.x, i) + hash2_term(v.y, i + 1) + hash2_term(v.z, i + 2) + hash2_term(v.w, i + 3);
        }
        done = n4 << 2;
    }
    for (int i = done + lane; i < a.E; i += 64) {
        h1 += gzsym::pick_term(b[i], (unsigned)i);
        h2 += hash2_term(b[i], (unsigned)i);
    }
    const u64 tag = make_tag(wave_sum(h1), wave_sum(h2));
    const u64 slot = slot_of(tag, a.N);
    const unsigned* e = a.table + slot * a.stride;
    const u64 e_tag = ((const u64*)e)[0], e_epoch = ((const u64*)e)[1];
    bool hit = e_epoch == a.epoch && ((e_tag ^ tag) & a.mask) == 0;
    if (hit) {                                   // (wave-uniform)
        const unsigned* p = e + entry_plane_off();
        int diff = 0;
        done = 0;
        if (aligned) {
            const int n4 = a.E >> 2;
            for (int i4 = lane; i4 < n4; i4 += 64) {
                const uint4 x = ((const uint4*)b)[i4], y = ((const uint4*)p)[i4];
                diff |= (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
            }
            done = n4 << 2;
        }
        for (int i = done + lane; i < a.E; i += 64) diff |= b[i] != p[i];
        hit = !__any(diff);
    }
    if (lane == 0) a.flags[row] = hit ? 0 : 1;
    if (!a.side) return;
    if (hit) {
        const float* o = (const float*)(e + entry_out_off(a.E));
        const int k = gzsym::pick_find_segment(a.sg, a.base + row);
        for (int j = lane; j < a.T; j += 64) {
            int role, m;
            gzsym::split_column(a.L, j, &role, &m);
            const int width = role < a.L.R ? a.L.P[role] : a.L.V;
            a.sg.out[k][role][(size_t)(a.base + row - a.sg.row0[k]) * width + m] = o[j];
        }
    } else if (lane == 0) {
        a.slot[row] = slot;
        a.tag[row] = tag;
        atomicMax(&a.claim[slot], claim_word(a.seq, row));
    }
}

// One wave per row: the row's rank among the misses (the flags before it, summed), the list of
// missed rows, their planes gathered into [n_miss][E]; the last row's wave writes n_miss.
__global__ void __launch_bounds__(256) cache_compact_kernel(const int* __restrict__ flags, int n, int E,
                                                            const unsigned* __restrict__ in, int* __restrict__ list,
                                                            unsigned* __restrict__ gather, int* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    unsigned before = 0;
    for (int i = lane; i < row; i += 64) before += (unsigned)flags[i];
    const int rank = (int)wave_sum(before);
    const int miss = flags[row];
    if (row == n - 1 && lane == 0) *count = rank + miss;
    if (!miss) return;
    if (lane == 0) list[rank] = row;
    wave_copy(gather + (size_t)rank * E, in + (size_t)row * E, E, lane);
}

// One wave per missed row: its raw outputs to the row's destinations and, if the row holds its
// slot's claim, the entry -- planes, outputs, the header last.
__global__ void __launch_bounds__(256) cache_fill_kernel(FillArgs a) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= a.nmiss) return;
    const int row = a.list[k];
    const u64 slot = a.slot[row];
    const bool winner = a.claim[slot] == claim_word(a.seq, row);
    unsigned* e = a.table + slot * a.stride;
    const u64 old_epoch = ((const u64*)e)[1];
    float* o = (float*)(e + entry_out_off(a.E));
    const int sgk = gzsym::pick_find_segment(a.sg, a.base + row);
    for (int j = lane; j < a.T; j += 64) {
        int role, m;
        gzsym::split_column(a.L, j, &role, &m);
        const int width = role < a.L.R ? a.L.P[role] : a.L.V;
        const float v = a.raw[role][(size_t)k * width + m];
        a.sg.out[sgk][role][(size_t)(a.base + row - a.sg.row0[sgk]) * width + m] = v;
        if (winner) o[j] = v;
    }
    if (!winner) return;
    wave_copy(e + entry_plane_off(), a.gather + (size_t)k * a.E, a.E, lane);
    __threadfence();
    if (lane == 0) {
        ((u64*)e)[0] = a.tag[row];
        ((u64*)e)[1] = a.epoch;
        atomicAdd(&a.counters[0], 1ull);
        if (old_epoch == a.epoch) atomicAdd(&a.counters[1], 1ull);
    }
}

static size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

static void release(gz_eval_cache* c) {
    (void)hipSetDevice(c->device);
    if (c->ev) { (void)hipEventSynchronize(c->ev); (void)hipEventDestroy(c->ev); }
    if (c->ev_count) (void)hipEventDestroy(c->ev_count);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    (void)hipFree(c->d_table);
    (void)hipFree(c->d_claim);
    (void)hipFree(c->d_flags);                   // (the scratch is one allocation)
    if (c->h_count) (void)hipHostFree(c->h_count);
    delete c;
}

extern "C" gz_eval_cache* gz_eval_cache_create(gz_net* net, long entries) {
    if (entries < 1) { set_error("eval cache: entries " + std::to_string(entries) + " (at least 1)"); return nullptr; }
    if (!net) { set_error("eval cache: null argument"); return nullptr; }
    NetView v;
    gzsym::net_view(net, &v);
    gz_eval_cache* c = new gz_eval_cache();
    c->net = net;
    c->device = v.device;
    c->N = (u64)entries;
    c->E = v.plane_elems;
    c->L.R = v.roles;
    c->L.V = v.num_values;
    c->L.S = 1;
    c->L.total = v.num_values;
    for (int r = 0; r < v.roles; ++r) { c->L.P[r] = v.policy[r]; c->L.total += v.policy[r]; }
    c->T = c->L.total;
    c->stride = entry_words(c->E, c->T);
    const char* eb = getenv("GZ_EVAL_CACHE_TAG_BITS");
    c->bits = tag_bits(eb ? atoi(eb) : 64, eb != nullptr);
    const char* ec = getenv("GZ_EVAL_CACHE_CHUNK_ROWS");
    c->chunk = chunk_rows(ec ? atoi(ec) : 0);
    const size_t entry_bytes = c->stride * 4 + 8;            // the entry and its claim word
    if ((u64)entries > (u64)kMaxTableBytes / entry_bytes) {
        set_error("eval cache: " + std::to_string(entries) + " entries of " + std::to_string(entry_bytes) + " bytes exceed the bound of " +
                  std::to_string(kMaxTableBytes) + " bytes");
        delete c;
        return nullptr;
    }
    // scratch: flags, list, slots, tags, count, gathered planes, raw outputs, host staging
    const size_t C = (size_t)c->chunk, E = (size_t)c->E, T = (size_t)c->T;
    const size_t o_list = align16(C * 4), o_slot = o_list + align16(C * 4), o_tag = o_slot + align16(C * 8),
                 o_count = o_tag + align16(C * 8), o_gather = o_count + 16, o_raw = o_gather + align16(C * E * 4),
                 o_io = o_raw + align16(C * T * 4), total = o_io + align16(C * (E + T) * 4);
    char* s = nullptr;
    bool ok = hipSetDevice(c->device) == hipSuccess && hipMalloc((void**)&c->d_table, (size_t)entries * c->stride * 4) == hipSuccess &&
              hipMalloc((void**)&c->d_claim, (size_t)entries * 8 + 16) == hipSuccess && hipMalloc((void**)&s, total) == hipSuccess;
    if (ok) {
        c->d_flags = (int*)s;
        c->d_list = (int*)(s + o_list);
        c->d_slot = (u64*)(s + o_slot);
        c->d_tag = (u64*)(s + o_tag);
        c->d_count = (int*)(s + o_count);
        c->d_gather = (float*)(s + o_gather);
        c->d_raw = (float*)(s + o_raw);
        c->d_io = (float*)(s + o_io);
        c->d_counters = c->d_claim + entries;    // (the two counters follow the claim words)
        ok = hipMemset(c->d_table, 0, (size_t)entries * c->stride * 4) == hipSuccess &&
             hipMemset(c->d_claim, 0, (size_t)entries * 8 + 16) == hipSuccess &&
             hipHostMalloc((void**)&c->h_count, sizeof(int)) == hipSuccess &&
             hipEventCreateWithFlags(&c->ev, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->ev_count, hipEventDisableTiming) == hipSuccess &&
             hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    }
    if (!ok) {
        set_error(std::string("eval cache: allocation of ") + std::to_string((size_t)entries * entry_bytes + total) +
                  " bytes: " + hipGetErrorString(hipGetLastError()));
        release(c);
        return nullptr;
    }
    c->net_epoch = net_epoch(net);
    return c;
}

extern "C" void gz_eval_cache_destroy(gz_eval_cache* c) {
    if (c) release(c);
}

static void flush(gz_eval_cache* c) {
    ++c->epoch;
    ++c->flushes;
}

extern "C" int gz_eval_cache_clear(gz_eval_cache* c) {
    if (!c) return set_error("eval cache: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    flush(c);
    return 0;
}

extern "C" int gz_eval_cache_stats(gz_eval_cache* c, struct gz_eval_cache_stats* out, int reset) {
    if (!c || !out) return set_error("eval cache: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    CACHECHK(hipSetDevice(c->device));
    CACHECHK(hipEventSynchronize(c->ev));
    u64 dev[2] = {0, 0};
    CACHECHK(hipMemcpy(dev, c->d_counters, sizeof dev, hipMemcpyDeviceToHost));
    out->calls = c->calls;
    out->rows = c->rows;
    out->hits = c->hits;
    out->forward_rows = c->forward_rows;
    out->inserts = (long)dev[0];
    out->replaced = (long)dev[1];
    out->flushes = c->flushes;
    out->entries = (long)c->N;
    out->entry_bytes = (long)(c->stride * 4);
    if (reset) {
        CACHECHK(hipMemset(c->d_counters, 0, sizeof dev));
        c->calls = c->rows = c->hits = c->forward_rows = c->flushes = 0;
    }
    return 0;
}

// the refusals of a call: nothing here touches the device
static int check_net(gz_net* net, gz_eval_cache* c, NetView* v) {
    if (net != c->net) return set_error("eval cache: made for another net");
    gzsym::net_view(net, v);
    if (v->device != c->device)
        return set_error("eval cache: made on device " + std::to_string(c->device) + ", the net is on device " + std::to_string(v->device));
    return 0;
}

// the destinations of a call with contiguous outputs: one segment
static PickSegments one_segment(const gz_eval_cache* c, float* const* d_pol, float* d_val) {
    PickSegments sg{};
    sg.nseg = 1;
    sg.row0[0] = 0;
    for (int r = 0; r < c->L.R; ++r) sg.out[0][r] = d_pol[r];
    sg.out[0][c->L.R] = d_val;
    return sg;
}

static void probe_launch(gz_eval_cache* c, hipStream_t stream, const float* d_in, int n, int side, int base,
                         const PickSegments& sg) {
    ProbeArgs a{};
    a.base = base;
    a.in = (const unsigned*)d_in;
    a.n = n;
    a.E = c->E;
    a.T = c->T;
    a.side = side;
    a.table = c->d_table;
    a.claim = c->d_claim;
    a.N = c->N;
    a.epoch = c->epoch;
    a.mask = tag_mask(c->bits);
    a.seq = c->seq;
    a.stride = c->stride;
    a.flags = c->d_flags;
    a.slot = c->d_slot;
    a.tag = c->d_tag;
    a.L = c->L;
    a.sg = sg;
    cache_probe_kernel<<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream>>>(a);
}

// rows [0, n) of d_planes through probe, compact, the net's forward of the misses and fill, chunk by
// chunk, on `stream` (c->mu held); row i's outputs go where `segs` says.  Blocks once per chunk, for
// the count of misses; `idle` (may be null) is called while it waits.
static int cached_chunks(gz_net* net, gz_eval_cache* c, hipStream_t stream, const float* d_planes, int n, const PickSegments& sg,
                         void (*idle)(void*) = nullptr, void* idle_arg = nullptr) {
    if (sg.nseg < 1 || sg.nseg > gzsym::kMaxPickSegments) return set_error("eval cache: " + std::to_string(sg.nseg) + " segments");
    CACHECHK(hipSetDevice(c->device));
    CACHECHK(hipStreamWaitEvent(stream, c->ev, 0));
    const u64 ne = net_epoch(net);
    if (ne != c->net_epoch) {
        flush(c);
        c->net_epoch = ne;
    }
    const int E = c->E;
    long hits = 0, fwd = 0;
    bool rolled = false;
    for (int r0 = 0; r0 < n && !rolled; r0 += c->chunk) {
        const int cn = std::min(c->chunk, n - r0);
        const float* in = d_planes + (size_t)r0 * E;
        ++c->seq;
        probe_launch(c, stream, in, cn, 1, r0, sg);
        CACHECHK(hipGetLastError());
        cache_compact_kernel<<<dim3((unsigned)((cn + 3) / 4)), dim3(256), 0, stream>>>(c->d_flags, cn, E, (const unsigned*)in, c->d_list,
                                                                                       (unsigned*)c->d_gather, c->d_count);
        CACHECHK(hipGetLastError());
        CACHECHK(hipMemcpyAsync(c->h_count, c->d_count, sizeof(int), hipMemcpyDeviceToHost, stream));
        CACHECHK(hipEventRecord(c->ev_count, stream));
        while (idle && hipEventQuery(c->ev_count) == hipErrorNotReady) idle(idle_arg);
        CACHECHK(hipEventSynchronize(c->ev_count));
        const int nmiss = *c->h_count;
        if (nmiss < 0 || nmiss > cn) return set_error("eval cache: miss count " + std::to_string(nmiss) + " of " + std::to_string(cn) + " rows");
        hits += cn - nmiss;
        fwd += nmiss;
        if (nmiss == 0) continue;
        FillArgs f{};
        float* raw[GZ_MAX_ROLES + 1];
        float* p = c->d_raw;
        for (int r = 0; r < c->L.R; ++r) { raw[r] = p; p += (size_t)nmiss * c->L.P[r]; }
        raw[c->L.R] = p;
        u64 fe = 0;
        gz_segment ms{};
        ms.rows = nmiss;
        ms.planes = c->d_gather;
        for (int r = 0; r < c->L.R; ++r) ms.policies[r] = raw[r];
        ms.values = raw[c->L.R];
        if (forward_segments_epoch(net, stream, &ms, 1, &fe)) return -1;
        if (fe != c->net_epoch) {                // a roll from another thread landed mid-call
            rolled = true;
            break;
        }
        f.nmiss = nmiss;
        f.base = r0;
        f.E = E;
        f.T = c->T;
        f.table = c->d_table;
        f.claim = c->d_claim;
        f.epoch = c->epoch;
        f.seq = c->seq;
        f.stride = c->stride;
        f.list = c->d_list;
        f.slot = c->d_slot;
        f.tag = c->d_tag;
        f.gather = (const unsigned*)c->d_gather;
        for (int r = 0; r <= c->L.R; ++r) f.raw[r] = raw[r];
        f.counters = c->d_counters;
        f.L = c->L;
        f.sg = sg;
        cache_fill_kernel<<<dim3((unsigned)((nmiss + 3) / 4)), dim3(256), 0, stream>>>(f);
        CACHECHK(hipGetLastError());
    }
    if (rolled) {
        // every row of the call through one forward, uncached: one weight generation for all of them
        u64 fe = 0;
        std::vector<gz_segment> gs((size_t)sg.nseg);
        for (int k = 0; k < sg.nseg; ++k) {
            gs[(size_t)k].rows = (k + 1 < sg.nseg ? sg.row0[k + 1] : n) - sg.row0[k];
            gs[(size_t)k].planes = d_planes + (size_t)sg.row0[k] * E;
            for (int r = 0; r < c->L.R; ++r) gs[(size_t)k].policies[r] = sg.out[k][r];
            gs[(size_t)k].values = sg.out[k][c->L.R];
        }
        if (forward_segments_epoch(net, stream, gs.data(), sg.nseg, &fe)) return -1;
        flush(c);
        c->net_epoch = fe;
        hits = 0;
        fwd = n;
    }
    CACHECHK(hipEventRecord(c->ev, stream));
    ++c->calls;
    c->rows += n;
    c->hits += hits;
    c->forward_rows += fwd;
    return 0;
}

extern "C" int gz_net_forward_cached_device(gz_net* net, gz_eval_cache* c, void* stream, const float* d_planes, int n,
                                            float* const* d_policies, float* d_values) {
    if (!net || !c || !d_planes || !d_policies || !d_values) return set_error("eval cache: null argument");
    NetView v;
    if (check_net(net, c, &v)) return -1;
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    return cached_chunks(net, c, (hipStream_t)stream, d_planes, n, one_segment(c, d_policies, d_values));
}

extern "C" int gz_net_forward_cached(gz_net* net, gz_eval_cache* c, const float* planes, int n, float* const* policies,
                                     float* values) {
    if (!net || !c || !planes || !policies || !values) return set_error("eval cache: null argument");
    NetView v;
    if (check_net(net, c, &v)) return -1;
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    CACHECHK(hipSetDevice(c->device));
    hipStream_t stream = (hipStream_t)v.host_stream;
    const size_t E = (size_t)c->E;
    for (int r0 = 0; r0 < n; r0 += c->chunk) {
        const int cn = std::min(c->chunk, n - r0);
        float* d_in = c->d_io;
        float* d_pol[GZ_MAX_ROLES];
        float* p = d_in + (size_t)cn * E;
        for (int r = 0; r < c->L.R; ++r) { d_pol[r] = p; p += (size_t)cn * c->L.P[r]; }
        float* d_val = p;
        CACHECHK(hipStreamWaitEvent(stream, c->ev, 0));
        CACHECHK(hipMemcpyAsync(d_in, planes + (size_t)r0 * E, (size_t)cn * E * sizeof(float), hipMemcpyHostToDevice, stream));
        if (cached_chunks(net, c, stream, d_in, cn, one_segment(c, d_pol, d_val))) return -1;
        --c->calls;                              // (one call, however many chunks)
        for (int r = 0; r < c->L.R; ++r)
            CACHECHK(hipMemcpyAsync(policies[r] + (size_t)r0 * c->L.P[r], d_pol[r], (size_t)cn * c->L.P[r] * sizeof(float),
                                    hipMemcpyDeviceToHost, stream));
        CACHECHK(hipMemcpyAsync(values + (size_t)r0 * c->L.V, d_val, (size_t)cn * c->L.V * sizeof(float), hipMemcpyDeviceToHost, stream));
        CACHECHK(hipStreamSynchronize(stream));  // (the staging is reused by the next chunk)
    }
    ++c->calls;
    return 0;
}

// The hit mask of planes [n][E] against the table as it stands: no claim, no copy, no flush (a net
// whose weight generation has moved since the last call reads as all misses, what the next call's
// flush will make of it).  Synchronous, on a stream of the cache's.
extern "C" int gz_eval_cache_probe(gz_eval_cache* c, int device_ptr, const float* planes, int n, int* hit) {
    if (!c || !planes || !hit) return set_error("eval cache: null argument");
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    CACHECHK(hipSetDevice(c->device));
    CACHECHK(hipEventSynchronize(c->ev));
    const bool stale = net_epoch(c->net) != c->net_epoch;
    const size_t E = (size_t)c->E;
    const PickSegments none{};
    for (int r0 = 0; r0 < n; r0 += c->chunk) {
        const int cn = std::min(c->chunk, n - r0);
        const float* src = planes + (size_t)r0 * E;
        if (!device_ptr) {
            CACHECHK(hipMemcpyAsync(c->d_io, src, (size_t)cn * E * sizeof(float), hipMemcpyHostToDevice, c->stream));
            src = c->d_io;
        }
        probe_launch(c, c->stream, src, cn, 0, 0, none);
        CACHECHK(hipGetLastError());
        CACHECHK(hipMemcpyAsync(hit + r0, c->d_flags, (size_t)cn * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        CACHECHK(hipStreamSynchronize(c->stream));
    }
    for (int i = 0; i < n; ++i) hit[i] = stale ? 0 : !hit[i];
    return 0;
}

// ---- the pieces the self-play runner uses (eval_cache.h) --------------------------------------------

int gzcache::runner_check(gz_net* net, gz_eval_cache* c) {
    NetView v;
    return check_net(net, c, &v);
}

int gzcache::cached_launch(gz_net* net, gz_eval_cache* c, hipStream_t stream, const float* d_planes, int n,
                           const gzsym::PickSegments& segs, void (*idle)(void*), void* idle_arg) {
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    return cached_chunks(net, c, stream, d_planes, n, segs, idle, idle_arg);
}
