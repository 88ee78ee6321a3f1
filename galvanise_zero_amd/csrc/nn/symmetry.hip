// The symmetry ensemble's two kernels and entry points (symmetry.h states the arithmetic; the net's
// own forward runs between the kernels, unchanged, through gz_net_forward_device).
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
    int scratch_rows = 0;                        // chunk rows the scratch holds
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
static int check_net(gz_net* net, gz_symmetry* s, NetView* v) {
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
    if (v->logits)
        return set_error("symmetry: the net is in gz_net_set_output_logits mode (an average of logits is not the ensemble)");
    return 0;
}

static size_t row_floats(const gz_symmetry* s) { return (size_t)s->E + (size_t)s->L.total; }

static int env_chunk_rows() {
    const char* e = getenv("GZ_SYM_CHUNK_ROWS");
    return e ? atoi(e) : 0;
}

// tables to the device (once) and scratch for chunks of `rows` rows
static int ensure_device(gz_symmetry* s, const NetView& v, int rows) {
    SYMCHK(hipSetDevice(s->device));
    if (!s->d_tables) {
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
    }
    if (rows > s->scratch_rows) {
        if (s->d_scratch) SYMCHK(hipFree(s->d_scratch));   // (waits for the work queued on it)
        s->d_scratch = nullptr;
        s->scratch_rows = 0;
        SYMCHK(hipMalloc((void**)&s->d_scratch, (size_t)s->L.S * rows * row_floats(s) * sizeof(float)));
        s->scratch_rows = rows;
    }
    return 0;
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
