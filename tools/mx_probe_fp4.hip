// Lab probe: operand / scale lane maps of v_mfma_scale_f32_16x16x128_f8f6f4 with an fp4 (e2m1) A operand and an fp8 (e4m3) B operand,
// found with one-hot operands; assumes only the C/D map.  Output: profiles/r14_mxfp4_lane_probe.log; what csrc/gemm_skinny.hip
// (gemm_skinny_mxfp4_kernel) relies on and tests/test_gpu_mxfp4.py pins with exact integers.
//   hipcc --offload-arch=gfx950 -O2 tools/mx_probe_fp4.hip -o tools/build/mx_probe_fp4
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

__global__ void mx_many(const v8i* a, const v8i* b, const int* sa, const int* sb, v4f* c) {
    const int l = threadIdx.x, p = blockIdx.x;
    v4f acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[p * 64 + l], b[p * 64 + l], acc, 4, 0, 0, sa[p * 64 + l], 0, sb[p * 64 + l]);
    c[p * 64 + l] = acc;
}

static float e4m3_decode(uint8_t v) {
    const int s = v >> 7, e = (v >> 3) & 15, m = v & 7;
    float x = e == 0 ? ldexpf((float)m / 8.f, -6) : ldexpf(1.f + (float)m / 8.f, e - 7);
    return s ? -x : x;
}

int main() {
    std::vector<uint8_t> code;
    for (int v = 0x08; v < 0x7F && code.size() < 64; ++v) code.push_back((uint8_t)v);
    for (int v = 0x88; v < 0xFF && code.size() < 128; ++v) code.push_back((uint8_t)v);
    const int P1 = 128;                     // probe p = (g, j): A nibble j (of 32, in the first 16 bytes) of every lane in group g = 1.0 (code 2)
    std::vector<uint8_t> A((size_t)P1 * 64 * 32, 0), B((size_t)P1 * 64 * 32, 0);
    std::vector<int> S((size_t)P1 * 64, 127);
    for (int p = 0; p < P1; ++p) {
        const int g = p >> 5, j = p & 31;
        for (int l = 0; l < 64; ++l) {
            if ((l >> 4) == g) A[((size_t)p * 64 + l) * 32 + j / 2] = (uint8_t)(2 << (4 * (j & 1)));
            for (int jb = 0; jb < 32; ++jb) B[((size_t)p * 64 + l) * 32 + jb] = code[(l >> 4) * 32 + jb];
        }
    }
    v8i *da, *db; int *ds, *ds2; v4f* dc;
    CK(hipMalloc(&da, A.size())); CK(hipMalloc(&db, B.size())); CK(hipMalloc(&ds, S.size() * 4)); CK(hipMalloc(&ds2, S.size() * 4));
    CK(hipMalloc(&dc, (size_t)P1 * 64 * 16));
    CK(hipMemcpy(da, A.data(), A.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(db, B.data(), B.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(ds, S.data(), S.size() * 4, hipMemcpyHostToDevice));
    mx_many<<<P1, 64>>>(da, db, ds, ds, dc);
    CK(hipDeviceSynchronize());
    std::vector<float> C((size_t)P1 * 256);
    CK(hipMemcpy(C.data(), dc, C.size() * 4, hipMemcpyDeviceToHost));
    printf("pairing: A fp4 (lane group g, nibble j) -> B fp8 (lane group, byte)\n");
    for (int p = 0; p < P1; ++p) {
        const float v00 = C[(size_t)p * 256];
        int hit = -1, uniform = 1;
        for (int q = 0; q < 128; ++q) if (e4m3_decode(code[q]) == v00) hit = q;
        for (int i = 0; i < 256; ++i) if (C[(size_t)p * 256 + i] != v00) uniform = 0;
        printf("  A(%d,%2d) -> B(%d,%2d) value %g%s\n", p >> 5, p & 31, hit < 0 ? -1 : hit >> 5, hit < 0 ? -1 : hit & 31, v00, uniform ? "" : " NOT UNIFORM");
    }
    // scale_a: lane L = 16 b (row 0, group b) doubled; A one-hot (g, j) in every row; B ones -> which (g, j) of row 0 come out as 2
    std::fill(B.begin(), B.end(), 0x38);
    CK(hipMemcpy(db, B.data(), B.size(), hipMemcpyHostToDevice));
    for (int b = 0; b < 4; ++b) {
        std::vector<int> SA((size_t)P1 * 64, 127);
        for (int p = 0; p < P1; ++p) SA[(size_t)p * 64 + 16 * b] = 128;
        CK(hipMemcpy(ds2, SA.data(), SA.size() * 4, hipMemcpyHostToDevice));
        mx_many<<<P1, 64>>>(da, db, ds2, ds, dc);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(C.data(), dc, C.size() * 4, hipMemcpyDeviceToHost));
        printf("scale_a lane %d doubles row 0 at A (g,j):", 16 * b);
        for (int p = 0; p < P1; ++p) {
            const float v = C[(size_t)p * 256];                   // row 0, col 0
            if (v == 2.f) printf(" (%d,%d)", p >> 5, p & 31); else if (v != 1.f) printf(" [%d,%d=%g]", p >> 5, p & 31, v);
        }
        printf("\n");
        int other = 0;
        for (int p = 0; p < P1; ++p) for (int i = 1; i < 4; ++i) if (C[(size_t)p * 256 + i] != 1.f) other = 1;    // rows 1..3, col 0: untouched
        printf("  rows 1..3 untouched: %s\n", other ? "NO" : "yes");
    }
    // scale_b: lane 16 b doubled; which A (g, j) (pairing through B) of column 0 come out as 2
    for (int b = 0; b < 4; ++b) {
        std::vector<int> SB((size_t)P1 * 64, 127);
        for (int p = 0; p < P1; ++p) SB[(size_t)p * 64 + 16 * b] = 128;
        CK(hipMemcpy(ds2, SB.data(), SB.size() * 4, hipMemcpyHostToDevice));
        mx_many<<<P1, 64>>>(da, db, ds, ds2, dc);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(C.data(), dc, C.size() * 4, hipMemcpyDeviceToHost));
        printf("scale_b lane %d doubles col 0 at A (g,j):", 16 * b);
        for (int p = 0; p < P1; ++p) {
            const float v = C[(size_t)p * 256];
            if (v == 2.f) printf(" (%d,%d)", p >> 5, p & 31); else if (v != 1.f) printf(" [%d,%d=%g]", p >> 5, p & 31, v);
        }
        printf("\n");
    }
    return 0;
}
