// v_mfma_f32_16x16x32_f16 probe for the fp16x3 conv (gzlayered::conv_f16_kernel), one wave:
//   map        the A / B / D lane maps the kernel assumes (bf16's: lane l holds A[l % 16][8 (l / 16) + j]
//              and B[8 (l / 16) + j][l % 16], register r of lane l is D[4 (l / 16) + r][l % 16]) against
//              an integer matrix product: small integers are exact in fp16 and fp32, so any other map
//              shows as a wrong integer
//   subnormal  whether fp16 subnormal inputs count: 2^-24 x 2^14 must give 2^-10, not 0
//   sum        how the 32 products of one instruction are summed: 2^24 + 31 x 1 (exact 16,777,247;
//              fp32 holds even numbers there), and 2^24 - 2^24 + 30 x 2^-10 (exact 0.029296875)
// Prints one line each; exits 1 when the map is not the assumed one.
// Build: hipcc -O3 --offload-arch=gfx950 -std=c++17 tools/probes/mfma_f16.hip -o tools/probes/mfma_f16.exe
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define CHK(x)                                                                    \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));          \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

// a [64][8], b [64][8] fragments as the lanes hold them; d [64][4]
__global__ void __launch_bounds__(64) mfma_kernel(const _Float16* a, const _Float16* b, float* d) {
    const int lane = threadIdx.x;
    const f16x8 av = *(const f16x8*)(a + lane * 8), bv = *(const f16x8*)(b + lane * 8);
    const f32x4 r = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    for (int i = 0; i < 4; ++i) d[lane * 4 + i] = r[i];
}

// D = A B of A [16][32], B [32][16] through the assumed lane maps
static std::vector<float> run(const std::vector<float>& A, const std::vector<float>& B) {
    std::vector<_Float16> fa(64 * 8), fb(64 * 8);
    for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
            fa[l * 8 + j] = (_Float16)A[(l & 15) * 32 + 8 * (l >> 4) + j];
            fb[l * 8 + j] = (_Float16)B[(8 * (l >> 4) + j) * 16 + (l & 15)];
        }
    _Float16 *da, *db;
    float* dd;
    CHK(hipMalloc((void**)&da, 64 * 8 * 2));
    CHK(hipMalloc((void**)&db, 64 * 8 * 2));
    CHK(hipMalloc((void**)&dd, 64 * 4 * 4));
    CHK(hipMemcpy(da, fa.data(), 64 * 8 * 2, hipMemcpyHostToDevice));
    CHK(hipMemcpy(db, fb.data(), 64 * 8 * 2, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(mfma_kernel, dim3(1), dim3(64), 0, 0, da, db, dd);
    CHK(hipDeviceSynchronize());
    std::vector<float> f(64 * 4), D(16 * 16);
    CHK(hipMemcpy(f.data(), dd, 64 * 4 * 4, hipMemcpyDeviceToHost));
    for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 4; ++r) D[(4 * (l >> 4) + r) * 16 + (l & 15)] = f[l * 4 + r];
    CHK(hipFree(da));
    CHK(hipFree(db));
    CHK(hipFree(dd));
    return D;
}

int main() {
    std::vector<float> A(16 * 32), B(32 * 16);
    for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 32; ++k) A[i * 32 + k] = (float)((i * 7 + k * 3 + (i * k) % 5) % 13 - 6);
    for (int k = 0; k < 32; ++k)
        for (int j = 0; j < 16; ++j) B[k * 16 + j] = (float)((k * 5 + j * 11 + (k * j) % 7) % 17 - 8);
    std::vector<float> D = run(A, B);
    int wrong = 0;
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) {
            float s = 0.f;
            for (int k = 0; k < 32; ++k) s += A[i * 32 + k] * B[k * 16 + j];
            wrong += D[i * 16 + j] != s;
        }
    std::printf("map: %d of 256 integer outputs differ from A B under the bf16 lane maps: %s\n", wrong, wrong ? "NOT the assumed map" : "ok");

    std::fill(A.begin(), A.end(), 0.f);
    std::fill(B.begin(), B.end(), 0.f);
    for (int i = 0; i < 16; ++i) A[i * 32] = std::ldexp(1.f, -24);
    for (int j = 0; j < 16; ++j) B[j] = 16384.f;
    D = run(A, B);
    std::printf("subnormal: 2^-24 x 2^14 = %.10g (2^-10 = %.10g): fp16 subnormal inputs %s\n", D[0], std::ldexp(1.f, -10),
                D[0] == std::ldexp(1.f, -10) ? "kept" : "FLUSHED");

    for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 32; ++k) A[i * 32 + k] = k == 0 ? 4096.f : 1.f;
    for (int k = 0; k < 32; ++k)
        for (int j = 0; j < 16; ++j) B[k * 16 + j] = k == 0 ? 4096.f : 1.f;
    D = run(A, B);
    std::printf("sum: 2^24 + 31 x 1 = %.1f (exact 16777247; fp32 neighbours 16777246, 16777248; 16777216 means the ones were dropped)\n", D[0]);
    for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 32; ++k) A[i * 32 + k] = k == 0 ? 4096.f : k == 1 ? -4096.f : 0.03125f;
    for (int k = 0; k < 32; ++k)
        for (int j = 0; j < 16; ++j) B[k * 16 + j] = k < 2 ? 4096.f : 0.03125f;
    D = run(A, B);
    std::printf("sum: 2^24 - 2^24 + 30 x 2^-10 = %.10g (exact 0.029296875)\n", D[0]);
    return wrong ? 1 : 0;
}
