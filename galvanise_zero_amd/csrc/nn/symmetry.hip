// The symmetry ensemble's two kernels and entry points, and below them the two kernels and entry
// points of the one-symmetry-per-row pick (symmetry.h states the arithmetic of both; the net's own
// forward runs between the kernels, unchanged, through gz_net_forward_device).  Last, the canonical
// orientation: its expand kernel and entry points (the gather is the pick's; with a cache the cached
// forward of eval_cache.hip runs between the kernels instead).
#include "eval_cache.h"
#include "symmetry.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>

using namespace gzsym;

#define SYMCHK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) return set_error(std::string("symmetry: " #x ": ") + hipGetErrorString(e_)); \
    } while (0)

struct gz_symmetry {
    int device = 0;
    OutLayout L{};
    int E = 0;
    std::vector<int> h_plane;                    // [S][E]
    std::vector<int> h_move[GZ_MAX_ROLES];       // [S][P_r]
    // device side, made by the first forward
    int* d_tables = nullptr;                     // the plane table, then each role's move table
    const int* d_plane = nullptr;
    const int* d_move[GZ_MAX_ROLES] = {};
    float* d_scratch = nullptr;                  // expanded planes and raw outputs of one chunk
    size_t scratch_floats = 0;                   // floats the scratch holds
    float* d_io = nullptr;                       // host entry point: a chunk's planes and results
    int io_rows = 0;
    std::mutex mu;                               // the host entry point: one call at a time
};

struct ReduceArgs {
    OutLayout L;
    int n;
    const float* raw[GZ_MAX_ROLES + 1];          // [S * n][P_r] per role; at index R the values [S * n][V]
    const int* src[GZ_MAX_ROLES];                // [S][P_r]
    float* out[GZ_MAX_ROLES + 1];                // [n][P_r] per role; at index R [n][V]
};

__global__ void __launch_bounds__(256) sym_expand_kernel(const float* __restrict__ in, float* __restrict__ out, int n, int E,
                                                         const int* __restrict__ plane_src, size_t total) {
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    out[o] = in[expand_src(o, n, E, plane_src)];
}

// one thread per output element: blockIdx.y is the row, blockIdx.x covers its sum P_r + V columns
__global__ void __launch_bounds__(256) sym_reduce_kernel(ReduceArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;
    if (j >= a.L.total || r >= a.n) return;
    int role, m;
    split_column(a.L, j, &role, &m);
    const int width = role < a.L.R ? a.L.P[role] : a.L.V;
    a.out[role][(size_t)r * width + m] = reduce_one(a.raw[role], role < a.L.R ? a.src[role] : nullptr, a.L.S, a.n, r, width, m);
}

extern "C" gz_symmetry* gz_symmetry_create(int device, int count, int plane_elems, const int* plane_src, int roles,
                                           const int* policy_sizes, const int* const* move_src) {
    const std::string err = validate_tables(count, plane_elems, plane_src, roles, policy_sizes, move_src);
    if (!err.empty()) {
        set_error(err);
        return nullptr;
    }
    gz_symmetry* s = new gz_symmetry();
    s->device = device;
    s->E = plane_elems;
    s->L.R = roles;
    s->L.S = count;
    s->L.V = 0;                                  // the net's, set by the first forward
    s->L.total = 0;
    s->h_plane.assign(plane_src, plane_src + (size_t)count * plane_elems);
    for (int r = 0; r < roles; ++r) {
        s->L.P[r] = policy_sizes[r];
        s->h_move[r].assign(move_src[r], move_src[r] + (size_t)count * policy_sizes[r]);
    }
    return s;
}

extern "C" void gz_symmetry_destroy(gz_symmetry* s) {
    if (!s) return;
    if (s->d_tables || s->d_scratch || s->d_io) {
        (void)hipSetDevice(s->device);
        (void)hipFree(s->d_tables);
        (void)hipFree(s->d_scratch);
        (void)hipFree(s->d_io);
    }
    delete s;
}

extern "C" int gz_symmetry_count(const gz_symmetry* s) { return s ? s->L.S : 0; }

// the refusals of a forward: nothing here touches the device
static int check_net(gz_net* net, gz_symmetry* s, NetView* v, bool allow_logits = false) {
    net_view(net, v);
    bool same = v->plane_elems == s->E && v->roles == s->L.R;
    for (int r = 0; same && r < s->L.R; ++r) same = v->policy[r] == s->L.P[r];
    if (!same) {
        std::string m = "symmetry: tables of plane_elems " + std::to_string(s->E) + ", policies";
        for (int r = 0; r < s->L.R; ++r) m += " " + std::to_string(s->L.P[r]);
        m += " are not the net's (plane_elems " + std::to_string(v->plane_elems) + ", policies";
        for (int r = 0; r < v->roles; ++r) m += " " + std::to_string(v->policy[r]);
        return set_error(m + ")");
    }
    if (v->device != s->device)
        return set_error("symmetry: tables made for device " + std::to_string(s->device) + ", the net is on device " +
                         std::to_string(v->device));
    if (s->L.total && v->num_values != s->L.V)
        return set_error("symmetry: tables in use with a net of " + std::to_string(s->L.V) + " values, this net has " +
                         std::to_string(v->num_values));
    if (v->logits && !allow_logits)
        return set_error("symmetry: the net is in gz_net_set_output_logits mode (an average of logits is not the ensemble)");
    return 0;
}

static size_t row_floats(const gz_symmetry* s) { return (size_t)s->E + (size_t)s->L.total; }

static int env_chunk_rows() {
    const char* e = getenv("GZ_SYM_CHUNK_ROWS");
    return e ? atoi(e) : 0;
}

// tables to the device (once)
static int ensure_tables(gz_symmetry* s, const NetView& v) {
    SYMCHK(hipSetDevice(s->device));
    if (s->d_tables) return 0;
    s->L.V = v.num_values;
    s->L.total = v.num_values;
    size_t ints = s->h_plane.size();
    for (int r = 0; r < s->L.R; ++r) { ints += s->h_move[r].size(); s->L.total += s->L.P[r]; }
    int* d = nullptr;
    SYMCHK(hipMalloc((void**)&d, ints * sizeof(int)));
    size_t off = 0;
    hipError_t e = hipMemcpy(d, s->h_plane.data(), s->h_plane.size() * sizeof(int), hipMemcpyHostToDevice);
    s->d_plane = d;
    off += s->h_plane.size();
    for (int r = 0; r < s->L.R && e == hipSuccess; ++r) {
        e = hipMemcpy(d + off, s->h_move[r].data(), s->h_move[r].size() * sizeof(int), hipMemcpyHostToDevice);
        s->d_move[r] = d + off;
        off += s->h_move[r].size();
    }
    if (e != hipSuccess) {
        (void)hipFree(d);
        return set_error(std::string("symmetry: table upload: ") + hipGetErrorString(e));
    }
    s->d_tables = d;
    return 0;
}

// the object's scratch, grown to `floats` floats: sized for the mode in use (the ensemble's S x rows
// expanded rows, or the pick path's rows with one int per row)
static int ensure_scratch(gz_symmetry* s, size_t floats) {
    if (floats <= s->scratch_floats) return 0;
    if (s->d_scratch) SYMCHK(hipFree(s->d_scratch));   // (waits for the work queued on it)
    s->d_scratch = nullptr;
    s->scratch_floats = 0;
    SYMCHK(hipMalloc((void**)&s->d_scratch, floats * sizeof(float)));
    s->scratch_floats = floats;
    return 0;
}

// tables to the device (once) and scratch for chunks of `rows` rows
static int ensure_device(gz_symmetry* s, const NetView& v, int rows) {
    if (ensure_tables(s, v)) return -1;
    return ensure_scratch(s, (size_t)s->L.S * rows * row_floats(s));
}

// rows [0, n) of d_planes through expand, the net's forward and reduce, chunk by chunk, on `stream`
static int forward_chunks(gz_net* net, gz_symmetry* s, const NetView& v, hipStream_t stream, const float* d_planes, int n,
                          float* const* d_pol, float* d_val) {
    const int S = s->L.S, E = s->E;
    const int chunk = chunk_rows(S, env_chunk_rows());
    if (ensure_device(s, v, std::min(n, chunk))) return -1;
    for (int r0 = 0; r0 < n; r0 += chunk) {
        const int c = std::min(chunk, n - r0);
        const size_t xr = (size_t)S * c;         // expanded rows of this chunk
        float* x = s->d_scratch;
        float* raw_pol[GZ_MAX_ROLES];
        float* p = x + xr * E;
        ReduceArgs a{};
        a.L = s->L;
        a.n = c;
        for (int r = 0; r < s->L.R; ++r) {
            raw_pol[r] = p;
            a.raw[r] = p;
            a.src[r] = s->d_move[r];
            a.out[r] = d_pol[r] + (size_t)r0 * s->L.P[r];
            p += xr * s->L.P[r];
        }
        float* raw_val = p;
        a.raw[s->L.R] = raw_val;
        a.out[s->L.R] = d_val + (size_t)r0 * s->L.V;
        const size_t total = xr * E;
        sym_expand_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(d_planes + (size_t)r0 * E, x, c, E,
                                                                                            s->d_plane, total);
        SYMCHK(hipGetLastError());
        if (gz_net_forward_device(net, stream, x, (int)xr, raw_pol, raw_val)) return -1;
        sym_reduce_kernel<<<dim3((unsigned)((s->L.total + 255) / 256), (unsigned)c), dim3(256), 0, stream>>>(a);
        SYMCHK(hipGetLastError());
    }
    return 0;
}

extern "C" int gz_net_forward_sym_device(gz_net* net, gz_symmetry* s, void* stream, const float* d_planes, int n,
                                         float* const* d_policies, float* d_values) {
    if (!net || !s || !d_planes || !d_policies || !d_values) return set_error("symmetry: null argument");
    NetView v;
    if (check_net(net, s, &v)) return -1;
    if (n <= 0) return 0;
    return forward_chunks(net, s, v, (hipStream_t)stream, d_planes, n, d_policies, d_values);
}

extern "C" int gz_net_forward_sym(gz_net* net, gz_symmetry* s, const float* planes, int n, float* const* policies,
                                  float* values) {
    if (!net || !s || !planes || !policies || !values) return set_error("symmetry: null argument");
    NetView v;
    if (check_net(net, s, &v)) return -1;
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(s->mu);
    hipStream_t stream = (hipStream_t)v.host_stream;
    const int chunk = chunk_rows(s->L.S, env_chunk_rows());
    if (ensure_device(s, v, std::min(n, chunk))) return -1;
    const int rows = std::min(n, chunk);
    if (rows > s->io_rows) {
        if (s->d_io) SYMCHK(hipFree(s->d_io));
        s->d_io = nullptr;
        s->io_rows = 0;
        SYMCHK(hipMalloc((void**)&s->d_io, (size_t)rows * row_floats(s) * sizeof(float)));
        s->io_rows = rows;
    }
    const size_t E = (size_t)s->E;
    for (int r0 = 0; r0 < n; r0 += chunk) {
        const int c = std::min(chunk, n - r0);
        float* d_in = s->d_io;
        float* d_pol[GZ_MAX_ROLES];
        float* p = d_in + (size_t)c * E;
        for (int r = 0; r < s->L.R; ++r) { d_pol[r] = p; p += (size_t)c * s->L.P[r]; }
        float* d_val = p;
        SYMCHK(hipMemcpyAsync(d_in, planes + (size_t)r0 * E, (size_t)c * E * sizeof(float), hipMemcpyHostToDevice, stream));
        if (forward_chunks(net, s, v, stream, d_in, c, d_pol, d_val)) return -1;
        for (int r = 0; r < s->L.R; ++r)
            SYMCHK(hipMemcpyAsync(policies[r] + (size_t)r0 * s->L.P[r], d_pol[r], (size_t)c * s->L.P[r] * sizeof(float),
                                  hipMemcpyDeviceToHost, stream));
        SYMCHK(hipMemcpyAsync(values + (size_t)r0 * s->L.V, d_val, (size_t)c * s->L.V * sizeof(float), hipMemcpyDeviceToHost,
                              stream));
    }
    SYMCHK(hipStreamSynchronize(stream));
    return 0;
}

// ---- one symmetry per row, picked from the row's own planes (symmetry.h states the definition) ----

struct GatherArgs {
    OutLayout L;
    int n;
    const int* picks;                            // [n]
    const float* raw[GZ_MAX_ROLES + 1];          // [n][P_r] per role; at index R the values [n][V]
    const int* src[GZ_MAX_ROLES];                // [S][P_r]
    PickSegments sg;
};

// One workgroup per row: the row's hash by wave shuffles and LDS (16-byte loads where E and the
// row's address allow, a scalar loop otherwise and for the tail), g to picks[row], then the row
// permuted through plane_src[g].  x == nullptr: the picks alone.
__global__ void __launch_bounds__(256) sym_pick_expand_kernel(const float* __restrict__ in, float* __restrict__ x,
                                                              int* __restrict__ picks, int n, int E, int S, unsigned salt,
                                                              const int* __restrict__ plane_src) {
    __shared__ unsigned part[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= n) return;
    const unsigned* b = (const unsigned*)in + (size_t)row * E;
    unsigned h = 0;
    int done = 0;
    if (((uintptr_t)b & 15) == 0) {
        const int n4 = E >> 2;
        for (int i4 = tid; i4 < n4; i4 += 256) {
            const uint4 v = ((const uint4*)b)[i4];
            const unsigned i = 4u * (unsigned)i4;
            h += pick_term(v.x, i) + pick_term(v.y, i + 1) + pick_term(v.z, i + 2) + pick_term(v.w, i + 3);
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < E; i += 256) h += pick_term(b[i], (unsigned)i);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) h += (unsigned)__shfl_xor((int)h, d, 64);
    if ((tid & 63) == 0) part[tid >> 6] = h;
    __syncthreads();
    const int g = pick_element(part[0] + part[1] + part[2] + part[3], salt, S);
    if (tid == 0) picks[row] = g;
    if (!x) return;
    for (int i = tid; i < E; i += 256) x[(size_t)row * E + i] = in[pick_expand_src(row, i, g, E, plane_src)];
}

// one thread per output element: blockIdx.y is the row, blockIdx.x covers its sum P_r + V columns
__global__ void __launch_bounds__(256) sym_pick_gather_kernel(GatherArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;
    if (j >= a.L.total || r >= a.n) return;
    int role, m;
    split_column(a.L, j, &role, &m);
    const int width = role < a.L.R ? a.L.P[role] : a.L.V;
    const int k = pick_find_segment(a.sg, r);
    a.sg.out[k][role][(size_t)(r - a.sg.row0[k]) * width + m] =
        a.raw[role][pick_gather_src(r, m, a.picks[r], width, role < a.L.R ? a.src[role] : nullptr)];
}

// the refusals of a pick forward: check_net's, except that a net in gz_net_set_output_logits mode is
// served (a permutation of logits is the logits of the permuted position; nothing is averaged)
int gzsym::pick_check(gz_net* net, gz_symmetry* s, NetView* v) { return check_net(net, s, v, true); }

int gzsym::pick_prepare(gz_symmetry* s, const NetView& v) {
    std::lock_guard<std::mutex> lk(s->mu);
    return ensure_tables(s, v);
}

int gzsym::pick_expand_launch(gz_symmetry* s, hipStream_t stream, unsigned salt, const float* d_in, int n, int* d_picks,
                              float* d_x) {
    if (n <= 0) return 0;
    sym_pick_expand_kernel<<<dim3((unsigned)n), dim3(256), 0, stream>>>(d_in, d_x, d_picks, n, s->E, s->L.S, salt, s->d_plane);
    SYMCHK(hipGetLastError());
    return 0;
}

int gzsym::pick_gather_launch(gz_symmetry* s, hipStream_t stream, const int* d_picks, int n, const float* const* d_raw,
                              const PickSegments& segs) {
    if (n <= 0) return 0;
    if (segs.nseg < 1 || segs.nseg > kMaxPickSegments) return set_error("symmetry: pick gather of " + std::to_string(segs.nseg) + " segments");
    GatherArgs a{};
    a.L = s->L;
    a.n = n;
    a.picks = d_picks;
    for (int r = 0; r <= s->L.R; ++r) a.raw[r] = d_raw[r];
    for (int r = 0; r < s->L.R; ++r) a.src[r] = s->d_move[r];
    a.sg = segs;
    sym_pick_gather_kernel<<<dim3((unsigned)((s->L.total + 255) / 256), (unsigned)n), dim3(256), 0, stream>>>(a);
    SYMCHK(hipGetLastError());
    return 0;
}

// rows [0, n) of d_planes through pick + expand, the net's forward and the gather, chunk by chunk
static int pick_chunks(gz_net* net, gz_symmetry* s, const NetView& v, unsigned salt, hipStream_t stream, const float* d_planes,
                       int n, float* const* d_pol, float* d_val) {
    const int E = s->E;
    const int chunk = chunk_rows(1, env_chunk_rows());
    if (ensure_tables(s, v)) return -1;
    const int rows = std::min(n, chunk);
    if (ensure_scratch(s, (size_t)rows * (row_floats(s) + 1))) return -1;   // + 1: the row's pick
    for (int r0 = 0; r0 < n; r0 += chunk) {
        const int c = std::min(chunk, n - r0);
        float* x = s->d_scratch;
        float* raw[GZ_MAX_ROLES + 1];
        float* p = x + (size_t)c * E;
        PickSegments sg{};
        sg.nseg = 1;
        sg.row0[0] = 0;
        for (int r = 0; r < s->L.R; ++r) {
            raw[r] = p;
            sg.out[0][r] = d_pol[r] + (size_t)r0 * s->L.P[r];
            p += (size_t)c * s->L.P[r];
        }
        raw[s->L.R] = p;
        sg.out[0][s->L.R] = d_val + (size_t)r0 * s->L.V;
        int* picks = (int*)(p + (size_t)c * s->L.V);
        if (pick_expand_launch(s, stream, salt, d_planes + (size_t)r0 * E, c, picks, x)) return -1;
        if (gz_net_forward_device(net, stream, x, c, raw, raw[s->L.R])) return -1;
        if (pick_gather_launch(s, stream, picks, c, raw, sg)) return -1;
    }
    return 0;
}

extern "C" int gz_net_forward_sym_pick_device(gz_net* net, gz_symmetry* s, unsigned salt, void* stream, const float* d_planes,
                                              int n, float* const* d_policies, float* d_values) {
    if (!net || !s || !d_planes || !d_policies || !d_values) return set_error("symmetry: null argument");
    NetView v;
    if (pick_check(net, s, &v)) return -1;
    if (n <= 0) return 0;
    return pick_chunks(net, s, v, salt, (hipStream_t)stream, d_planes, n, d_policies, d_values);
}

// a chunk's planes and results of the host entry points
static int ensure_io(gz_symmetry* s, int rows) {
    if (rows <= s->io_rows) return 0;
    if (s->d_io) SYMCHK(hipFree(s->d_io));
    s->d_io = nullptr;
    s->io_rows = 0;
    SYMCHK(hipMalloc((void**)&s->d_io, (size_t)rows * row_floats(s) * sizeof(float)));
    s->io_rows = rows;
    return 0;
}

extern "C" int gz_net_forward_sym_pick(gz_net* net, gz_symmetry* s, unsigned salt, const float* planes, int n,
                                       float* const* policies, float* values) {
    if (!net || !s || !planes || !policies || !values) return set_error("symmetry: null argument");
    NetView v;
    if (pick_check(net, s, &v)) return -1;
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(s->mu);
    hipStream_t stream = (hipStream_t)v.host_stream;
    const int chunk = chunk_rows(1, env_chunk_rows());
    if (ensure_tables(s, v) || ensure_io(s, std::min(n, chunk))) return -1;
    const size_t E = (size_t)s->E;
    for (int r0 = 0; r0 < n; r0 += chunk) {
        const int c = std::min(chunk, n - r0);
        float* d_in = s->d_io;
        float* d_pol[GZ_MAX_ROLES];
        float* p = d_in + (size_t)c * E;
        for (int r = 0; r < s->L.R; ++r) { d_pol[r] = p; p += (size_t)c * s->L.P[r]; }
        float* d_val = p;
        SYMCHK(hipMemcpyAsync(d_in, planes + (size_t)r0 * E, (size_t)c * E * sizeof(float), hipMemcpyHostToDevice, stream));
        if (pick_chunks(net, s, v, salt, stream, d_in, c, d_pol, d_val)) return -1;
        for (int r = 0; r < s->L.R; ++r)
            SYMCHK(hipMemcpyAsync(policies[r] + (size_t)r0 * s->L.P[r], d_pol[r], (size_t)c * s->L.P[r] * sizeof(float),
                                  hipMemcpyDeviceToHost, stream));
        SYMCHK(hipMemcpyAsync(values + (size_t)r0 * s->L.V, d_val, (size_t)c * s->L.V * sizeof(float), hipMemcpyDeviceToHost,
                              stream));
    }
    SYMCHK(hipStreamSynchronize(stream));
    return 0;
}

// The g of each row as sym_pick_expand_kernel computes it (no net: the hash needs the planes alone).
// Synchronous, on the null stream, through buffers of its own.
extern "C" int gz_symmetry_picks(gz_symmetry* s, unsigned salt, int device_ptr, const float* planes, int n, int* out) {
    if (!s || !planes || !out) return set_error("symmetry: null argument");
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(s->mu);
    SYMCHK(hipSetDevice(s->device));
    const size_t E = (size_t)s->E;
    const int chunk = std::min(n, chunk_rows(1, env_chunk_rows()));
    char* mem = nullptr;
    const size_t pick_bytes = ((size_t)chunk * sizeof(int) + 15) & ~(size_t)15;
    SYMCHK(hipMalloc((void**)&mem, pick_bytes + (device_ptr ? 0 : (size_t)chunk * E * sizeof(float))));
    int* d_picks = (int*)mem;
    float* d_in = (float*)(mem + pick_bytes);
    hipError_t e = hipSuccess;
    for (int r0 = 0; r0 < n && e == hipSuccess; r0 += chunk) {
        const int c = std::min(chunk, n - r0);
        const float* src = planes + (size_t)r0 * E;
        if (!device_ptr) {
            e = hipMemcpy(d_in, src, (size_t)c * E * sizeof(float), hipMemcpyHostToDevice);
            src = d_in;
        }
        if (e != hipSuccess) break;
        sym_pick_expand_kernel<<<dim3((unsigned)c), dim3(256), 0, 0>>>(src, nullptr, d_picks, c, s->E, s->L.S, salt, nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(out + r0, d_picks, (size_t)c * sizeof(int), hipMemcpyDeviceToHost);
    }
    (void)hipFree(mem);
    if (e != hipSuccess) return set_error(std::string("symmetry: picks: ") + hipGetErrorString(e));
    return 0;
}

// ---- canonical orientation (symmetry.h states the definition) -------------------------------------

__device__ inline unsigned canon_wave_sum(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

// One workgroup per row.  kLds: the row is read once into LDS (16-byte loads where the row is 16-byte
// aligned, a scalar loop otherwise and for the tail) and every image is gathered from there; else
// (a row over kCanonLdsWords) the images are gathered from global memory.  Thread tid takes elements
// tid, tid + 256, ... of every image -- the tables are read coalesced -- and keeps the 2 S partial
// sums of the two hashes; wave shuffles, then the four waves through LDS, give the totals, from which
// every thread computes g (canon_pick).  picks[row] = g, tags[row] = t_g (tags may be null), and the
// row permuted through plane_src[g] to x (x == nullptr: g and the tag alone).
template <bool kLds>
__global__ void __launch_bounds__(256) sym_canon_expand_kernel(const float* __restrict__ in, float* __restrict__ x,
                                                               int* __restrict__ picks, unsigned long long* __restrict__ tags,
                                                               int n, int E, int S, unsigned salt,
                                                               const int* __restrict__ plane_src) {
    extern __shared__ uint4 canon_row4[];        // kLds: the row's E words
    __shared__ unsigned part[4][2 * kMaxCount];
    __shared__ unsigned tot[2 * kMaxCount];      // h1 of elements 0 .. 7, then h2
    // static LDS precedes the dynamic region unpadded: its size keeps the row's 16-byte stores aligned
    static_assert((sizeof(part) + sizeof(tot)) % 16 == 0, "the dynamic LDS row must start 16-byte aligned");
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= n) return;
    const unsigned* b = (const unsigned*)in + (size_t)row * E;
    const unsigned* src = b;
    if (kLds) {
        unsigned* lrow = (unsigned*)canon_row4;
        int done = 0;
        if (((uintptr_t)b & 15) == 0) {
            const int n4 = E >> 2;
            for (int i4 = tid; i4 < n4; i4 += 256) canon_row4[i4] = ((const uint4*)b)[i4];
            done = n4 << 2;
        }
        for (int i = done + tid; i < E; i += 256) lrow[i] = b[i];
        __syncthreads();
        src = lrow;
    }
    unsigned h1[kMaxCount] = {}, h2[kMaxCount] = {};
    for (int i = tid; i < E; i += 256) {
#pragma unroll
        for (int s = 0; s < kMaxCount; ++s)
            if (s < S) {
                const unsigned v = src[plane_src[(size_t)s * E + i]];
                h1[s] += pick_term(v, (unsigned)i);
                h2[s] += gzcache::hash2_term(v, (unsigned)i);
            }
    }
#pragma unroll
    for (int s = 0; s < kMaxCount; ++s)
        if (s < S) {                             // (uniform)
            h1[s] = canon_wave_sum(h1[s]);
            h2[s] = canon_wave_sum(h2[s]);
        }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int s = 0; s < kMaxCount; ++s) {
            part[tid >> 6][s] = h1[s];
            part[tid >> 6][kMaxCount + s] = h2[s];
        }
    }
    __syncthreads();
    if (tid < 2 * kMaxCount) tot[tid] = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
    __syncthreads();
    unsigned long long tag;
    const int g = canon_pick(tot, tot + kMaxCount, S, salt, &tag);
    if (tid == 0) {
        picks[row] = g;
        if (tags) tags[row] = tag;
    }
    if (!x) return;
    for (int i = tid; i < E; i += 256) x[(size_t)row * E + i] = __uint_as_float(src[plane_src[(size_t)g * E + i]]);
}

static int canon_launch(hipStream_t stream, unsigned salt, const float* d_in, int n, int E, int S, const int* d_plane,
                        int* d_picks, unsigned long long* d_tags, float* d_x) {
    if (n <= 0) return 0;
    if (E <= kCanonLdsWords)
        sym_canon_expand_kernel<true><<<dim3((unsigned)n), dim3(256), (((size_t)E + 3) & ~(size_t)3) * 4, stream>>>(
            d_in, d_x, d_picks, d_tags, n, E, S, salt, d_plane);
    else
        sym_canon_expand_kernel<false><<<dim3((unsigned)n), dim3(256), 0, stream>>>(d_in, d_x, d_picks, d_tags, n, E, S, salt,
                                                                                    d_plane);
    SYMCHK(hipGetLastError());
    return 0;
}

int gzsym::canon_expand_launch(gz_symmetry* s, hipStream_t stream, unsigned salt, const float* d_in, int n, int* d_picks,
                               unsigned long long* d_tags, float* d_x) {
    return canon_launch(stream, salt, d_in, n, s->E, s->L.S, s->d_plane, d_picks, d_tags, d_x);
}

// the refusals of a canonical forward, no device call: the pick's, and with a cache the cache's
static int canon_check(gz_net* net, gz_symmetry* s, gz_eval_cache* cache, NetView* v) {
    if (pick_check(net, s, v)) return -1;
    return cache ? gzcache::runner_check(net, cache) : 0;
}

// pick_chunks with the canonical expand; between expand and gather the net's forward of the canonical
// planes, or with a cache one cached call of them, its one segment the raw scratch
static int canon_chunks(gz_net* net, gz_symmetry* s, const NetView& v, unsigned salt, gz_eval_cache* cache, hipStream_t stream,
                        const float* d_planes, int n, float* const* d_pol, float* d_val) {
    const int E = s->E;
    const int chunk = chunk_rows(1, env_chunk_rows());
    if (ensure_tables(s, v)) return -1;
    const int rows = std::min(n, chunk);
    if (ensure_scratch(s, (size_t)rows * (row_floats(s) + 1))) return -1;   // + 1: the row's element
    for (int r0 = 0; r0 < n; r0 += chunk) {
        const int c = std::min(chunk, n - r0);
        float* x = s->d_scratch;
        float* raw[GZ_MAX_ROLES + 1];
        float* p = x + (size_t)c * E;
        PickSegments sg{}, rawsg{};
        sg.nseg = rawsg.nseg = 1;
        sg.row0[0] = rawsg.row0[0] = 0;
        for (int r = 0; r < s->L.R; ++r) {
            raw[r] = p;
            rawsg.out[0][r] = p;
            sg.out[0][r] = d_pol[r] + (size_t)r0 * s->L.P[r];
            p += (size_t)c * s->L.P[r];
        }
        raw[s->L.R] = p;
        rawsg.out[0][s->L.R] = p;
        sg.out[0][s->L.R] = d_val + (size_t)r0 * s->L.V;
        int* picks = (int*)(p + (size_t)c * s->L.V);
        if (canon_expand_launch(s, stream, salt, d_planes + (size_t)r0 * E, c, picks, nullptr, x)) return -1;
        if (cache) {
            if (gzcache::cached_launch(net, cache, stream, x, c, rawsg, nullptr, nullptr)) return -1;
        } else if (gz_net_forward_device(net, stream, x, c, raw, raw[s->L.R])) {
            return -1;
        }
        if (pick_gather_launch(s, stream, picks, c, raw, sg)) return -1;
    }
    return 0;
}

extern "C" int gz_net_forward_sym_canon_device(gz_net* net, gz_symmetry* s, unsigned salt, gz_eval_cache* cache, void* stream,
                                               const float* d_planes, int n, float* const* d_policies, float* d_values) {
    if (!net || !s || !d_planes || !d_policies || !d_values) return set_error("symmetry: null argument");
    NetView v;
    if (canon_check(net, s, cache, &v)) return -1;
    if (n <= 0) return 0;
    return canon_chunks(net, s, v, salt, cache, (hipStream_t)stream, d_planes, n, d_policies, d_values);
}

extern "C" int gz_net_forward_sym_canon(gz_net* net, gz_symmetry* s, unsigned salt, gz_eval_cache* cache, const float* planes,
                                        int n, float* const* policies, float* values) {
    if (!net || !s || !planes || !policies || !values) return set_error("symmetry: null argument");
    NetView v;
    if (canon_check(net, s, cache, &v)) return -1;
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(s->mu);
    hipStream_t stream = (hipStream_t)v.host_stream;
    const int chunk = chunk_rows(1, env_chunk_rows());
    if (ensure_tables(s, v) || ensure_io(s, std::min(n, chunk))) return -1;
    const size_t E = (size_t)s->E;
    for (int r0 = 0; r0 < n; r0 += chunk) {
        const int c = std::min(chunk, n - r0);
        float* d_in = s->d_io;
        float* d_pol[GZ_MAX_ROLES];
        float* p = d_in + (size_t)c * E;
        for (int r = 0; r < s->L.R; ++r) { d_pol[r] = p; p += (size_t)c * s->L.P[r]; }
        float* d_val = p;
        SYMCHK(hipMemcpyAsync(d_in, planes + (size_t)r0 * E, (size_t)c * E * sizeof(float), hipMemcpyHostToDevice, stream));
        if (canon_chunks(net, s, v, salt, cache, stream, d_in, c, d_pol, d_val)) return -1;
        for (int r = 0; r < s->L.R; ++r)
            SYMCHK(hipMemcpyAsync(policies[r] + (size_t)r0 * s->L.P[r], d_pol[r], (size_t)c * s->L.P[r] * sizeof(float),
                                  hipMemcpyDeviceToHost, stream));
        SYMCHK(hipMemcpyAsync(values + (size_t)r0 * s->L.V, d_val, (size_t)c * s->L.V * sizeof(float), hipMemcpyDeviceToHost,
                              stream));
    }
    SYMCHK(hipStreamSynchronize(stream));
    return 0;
}

// g and t_g of each row as sym_canon_expand_kernel computes them (no net: the planes and the plane
// table alone).  Synchronous, on the null stream, through buffers of its own.
extern "C" int gz_symmetry_canon(gz_symmetry* s, unsigned salt, int device_ptr, const float* planes, int n, int* g_out,
                                 unsigned long long* tag_out) {
    if (!s || !planes || !g_out) return set_error("symmetry: null argument");
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(s->mu);
    SYMCHK(hipSetDevice(s->device));
    const size_t E = (size_t)s->E;
    const int chunk = std::min(n, chunk_rows(1, env_chunk_rows()));
    auto pad = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t tag_bytes = pad((size_t)chunk * sizeof(unsigned long long)), pick_bytes = pad((size_t)chunk * sizeof(int)),
                 table_bytes = s->d_plane ? 0 : pad(s->h_plane.size() * sizeof(int));
    char* mem = nullptr;
    SYMCHK(hipMalloc((void**)&mem, tag_bytes + pick_bytes + table_bytes + (device_ptr ? 0 : (size_t)chunk * E * sizeof(float))));
    unsigned long long* d_tags = (unsigned long long*)mem;
    int* d_picks = (int*)(mem + tag_bytes);
    const int* d_plane = s->d_plane;
    float* d_in = (float*)(mem + tag_bytes + pick_bytes + table_bytes);
    hipError_t e = hipSuccess;
    if (!d_plane) {                              // (no forward has uploaded the tables yet)
        e = hipMemcpy(mem + tag_bytes + pick_bytes, s->h_plane.data(), s->h_plane.size() * sizeof(int), hipMemcpyHostToDevice);
        d_plane = (const int*)(mem + tag_bytes + pick_bytes);
    }
    int rc = 0;
    for (int r0 = 0; r0 < n && e == hipSuccess && rc == 0; r0 += chunk) {
        const int c = std::min(chunk, n - r0);
        const float* src = planes + (size_t)r0 * E;
        if (!device_ptr) {
            e = hipMemcpy(d_in, src, (size_t)c * E * sizeof(float), hipMemcpyHostToDevice);
            src = d_in;
        }
        if (e != hipSuccess) break;
        rc = canon_launch(0, salt, src, c, s->E, s->L.S, d_plane, d_picks, d_tags, nullptr);
        if (rc) break;
        e = hipMemcpy(g_out + r0, d_picks, (size_t)c * sizeof(int), hipMemcpyDeviceToHost);
        if (e == hipSuccess && tag_out) e = hipMemcpy(tag_out + r0, d_tags, (size_t)c * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    }
    (void)hipFree(mem);
    if (rc) return -1;
    if (e != hipSuccess) return set_error(std::string("symmetry: canon: ") + hipGetErrorString(e));
    return 0;
}
