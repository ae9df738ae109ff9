// Field- and scalar-arithmetic self-test entry points (tests/test_field_gpu.py,
// tests/test_scalar_gpu.py): run one device operation over caller-supplied operands so the
// inline-asm carry chains -- including their rare wave-uniform fold branches -- and the mod-n
// reduction's folds and conditional subtractions are checked against Python big integers.
#include "gpu_common.h"
#include "secp256k1_device.h"

namespace bcc {

__global__ __launch_bounds__(256) void fe_selftest_kernel(int op, const u32* __restrict__ a,
                                                          const u32* __restrict__ b,
                                                          u32* __restrict__ out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe x, y, r;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        x.v[j] = a[i * 8 + j];
        y.v[j] = b[i * 8 + j];
    }
    r = fe_zero();
    switch (op) {
        case 0: fe_add(r, x, y); break;
        case 1: fe_sub(r, x, y); break;
        case 2: fe_mul(r, x, y); break;
        case 3: fe_sqr(r, x); break;
        case 4: fe_shl<1>(r, x); break;
        case 5: fe_shl<2>(r, x); break;
        case 6: fe_shl<3>(r, x); break;
        case 7: fe_neg(r, x); break;
        case 8: r.v[0] = fe_is_zero(x) ? 1u : 0u; break;
        case 9: r = x; fe_normalize(r); break;
        case 10: fe_inv(r, x); break;  // weak input, normalized inverse
        case 11: {                     // scalar inverse of x < n
            sc xs, rs;
#pragma unroll
            for (int j = 0; j < 8; j++) xs.v[j] = x.v[j];
            sc_inv(rs, xs);
#pragma unroll
            for (int j = 0; j < 8; j++) r.v[j] = rs.v[j];
            break;
        }
        default: break;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) out[i * 8 + j] = r.v[j];
}

// Scalar (mod n) self-test: the same pattern over sc_mul / sc_sqr (the exact product columns and
// the sc_mac / sc_reduce512 folds), sc_add, sc_neg, sc_mul_shift_384, sc_split_lambda, and fe_sqrt.
__global__ __launch_bounds__(256) void sc_selftest_kernel(int op, const u32* __restrict__ a,
                                                          const u32* __restrict__ b,
                                                          u32* __restrict__ out,
                                                          u32* __restrict__ out2, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    sc x, y, r, r2;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        x.v[j] = a[i * 8 + j];
        y.v[j] = b[i * 8 + j];
        r.v[j] = 0;
        r2.v[j] = 0;
    }
    switch (op) {
        case 0: sc_mul(r, x, y); break;
        case 1: sc_sqr(r, x); break;
        case 2: sc_add(r, x, y); break;
        case 3: sc_neg(r, x); break;
        case 4: {
            const u32 G1[8] = BCC_G1_LIMBS;
            sc_mul_shift_384(r, x, G1);
            break;
        }
        case 5: {
            const u32 G2[8] = BCC_G2_LIMBS;
            sc_mul_shift_384(r, x, G2);
            break;
        }
        case 6: sc_split_lambda(r, r2, x); break;
        case 7: {  // weak field input; the root normalized, the returned bool in out2[0]
            fe fx, fr;
#pragma unroll
            for (int j = 0; j < 8; j++) fx.v[j] = x.v[j];
            r2.v[0] = fe_sqrt(fr, fx) ? 1u : 0u;
            fe_normalize(fr);
#pragma unroll
            for (int j = 0; j < 8; j++) r.v[j] = fr.v[j];
            break;
        }
        default: break;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        out[i * 8 + j] = r.v[j];
        out2[i * 8 + j] = r2.v[j];
    }
}

}  // namespace bcc

extern "C" {

// a, b, out: n x 8 little-endian u32 limbs (host memory).  op: 0 add, 1 sub, 2 mul, 3 sqr,
// 4/5/6 shift left by 1/2/3, 7 neg, 8 is_zero (out[0]), 9 normalize, 10 fe_inv, 11 sc_inv (a < n).
// 0 on success.
int mi_fe_selftest(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
    using namespace bcc;
    if (n == 0) return 0;
    size_t bytes = n * 32;
    u32 *da = nullptr, *db = nullptr, *dout = nullptr;
    BCC_HIP_TRY(hipMalloc(&da, bytes));
    BCC_HIP_TRY(hipMalloc(&db, bytes));
    BCC_HIP_TRY(hipMalloc(&dout, bytes));
    BCC_HIP_TRY(hipMemcpy(da, a, bytes, hipMemcpyHostToDevice));
    BCC_HIP_TRY(hipMemcpy(db, b, bytes, hipMemcpyHostToDevice));
    unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(fe_selftest_kernel, dim3(grid), dim3(256), 0, 0, op, da, db, dout, n);
    BCC_HIP_TRY(hipGetLastError());
    BCC_HIP_TRY(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    (void)hipFree(da);
    (void)hipFree(db);
    (void)hipFree(dout);
    return 0;
}

// a, b, out, out2: n x 8 little-endian u32 limbs (host memory).  op: 0 sc_mul (any 256-bit a, b),
// 1 sc_sqr, 2 sc_add (a, b < n), 3 sc_neg (a < n), 4 / 5 sc_mul_shift_384 by g1 / g2,
// 6 sc_split_lambda (out = k1, out2 = k2), 7 fe_sqrt (weak a: out = the root normalized,
// out2[0] = the returned bool).  out2 is zero for the other ops.  0 on success.
int mi_sc_selftest(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* out2,
                   size_t n) {
    using namespace bcc;
    if (n == 0) return 0;
    if (op < 0 || op > 7) return -1;
    size_t bytes = n * 32;
    u32 *da = nullptr, *db = nullptr, *dout = nullptr, *dout2 = nullptr;
    BCC_HIP_TRY(hipMalloc(&da, bytes));
    BCC_HIP_TRY(hipMalloc(&db, bytes));
    BCC_HIP_TRY(hipMalloc(&dout, bytes));
    BCC_HIP_TRY(hipMalloc(&dout2, bytes));
    BCC_HIP_TRY(hipMemcpy(da, a, bytes, hipMemcpyHostToDevice));
    BCC_HIP_TRY(hipMemcpy(db, b, bytes, hipMemcpyHostToDevice));
    unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(sc_selftest_kernel, dim3(grid), dim3(256), 0, 0, op, da, db, dout, dout2, n);
    BCC_HIP_TRY(hipGetLastError());
    BCC_HIP_TRY(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    BCC_HIP_TRY(hipMemcpy(out2, dout2, bytes, hipMemcpyDeviceToHost));
    (void)hipFree(da);
    (void)hipFree(db);
    (void)hipFree(dout);
    (void)hipFree(dout2);
    return 0;
}

// The device's compute-unit count (hipDeviceAttributeMultiprocessorCount, the figure the kernels'
// launch shapes and the latency-mode threshold of small ECDSA rounds are derived from), so tests
// can size a batch on either side of that threshold.  Negative on error.
int mi_device_cus(int device) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return cus;
}

}  // extern "C"
