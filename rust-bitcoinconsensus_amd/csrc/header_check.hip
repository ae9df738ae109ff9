// Header chains on the GPU: the kernels and the device rounds of bcc_headers_batch and
// mi_pow_check_tuples (include/bcc_amd.h).  The lane code and the records are header_check.h; the
// host pass is host/headers.cpp.
//
//   K_hhash  header_hash_kernel     one lane per header: five 16-byte loads, SHA-256d of the 80
//                                   bytes in registers (two compressions and the digest's own),
//                                   the target from nBits, target against pow_limit and hash
//                                   against target; writes the hash row and the proof-of-work byte.
//   K_hctx   header_context_kernel  one lane per header, behind K_hhash on the round's stream:
//                                   linkage against hash row i - 1, the expected nBits (a retarget
//                                   on a boundary), the median of the eleven times before, the
//                                   upper time bound, the version gates; writes the status word.
//                                   Rows and times before the round's first header come from the
//                                   round's context record.
//   K_pow    pow_check_kernel       mi_pow_check_tuples: K_hhash's comparison over given rows.
// The host half lives here rather than under csrc/host because it launches kernels.
#include "header_check.h"
#include "gpu_common.h"
#include "host/tuples.h"

namespace bcc {

__global__ __launch_bounds__(256) void header_hash_kernel(const uint4* __restrict__ hdr, uint32_t n,
                                                          const HeaderRoundCtx* __restrict__ ctx,
                                                          uint4* __restrict__ hashes,
                                                          uint8_t* __restrict__ pow_ok) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t h[HEADER_WORDS], d[8];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const uint4 v = hdr[5 * (size_t)i + k];
        h[4 * k] = v.x;
        h[4 * k + 1] = v.y;
        h[4 * k + 2] = v.z;
        h[4 * k + 3] = v.w;
    }
    header_hash_lane(h, d);
    hashes[2 * (size_t)i] = make_uint4(d[0], d[1], d[2], d[3]);
    hashes[2 * (size_t)i + 1] = make_uint4(d[4], d[5], d[6], d[7]);
    pow_ok[i] = pow_check(d, h[HW_BITS], ctx->pow_limit) ? 1 : 0;
}

__global__ __launch_bounds__(256) void header_context_kernel(const uint8_t* __restrict__ hdr, uint32_t n,
                                                             const HeaderRoundCtx* __restrict__ ctx,
                                                             const uint32_t* __restrict__ hashes,
                                                             const uint8_t* __restrict__ pow_ok,
                                                             int* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    status[i] = header_context_lane(hdr, hashes, pow_ok, i, *ctx);
}

struct PowLimit {
    uint32_t w[8];
};
__global__ __launch_bounds__(256) void pow_check_kernel(const uint4* __restrict__ hash,
                                                        const uint32_t* __restrict__ bits, uint32_t n,
                                                        PowLimit limit, uint8_t* __restrict__ ok) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 a = hash[2 * (size_t)i], b = hash[2 * (size_t)i + 1];
    const uint32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    ok[i] = pow_check(d, bits[i], limit.w) ? 1 : 0;
}

namespace {

// Rows of one device round: the records' indices are 32-bit and the arena goes up in one copy.
constexpr size_t HEADER_ROUND_MAX = (size_t)1 << 24;

const bool g_timing = [] {
    const char* e = getenv("BCC_HEADER_TIMING");
    return e && atoi(e) != 0;
}();
thread_local double tl_ms[HEADER_MS_COUNT];

int header_round(int device, HeaderRound& r) {
    const size_t n = r.n;
    // every index a kernel will use, before anything is launched
    if (n == 0 || n > HEADER_ROUND_MAX || r.ctx.interval == 0 || r.ctx.n_times > MTP_SPAN)
        return (int)hipErrorInvalidValue;
    // uploaded: context | headers;  downloaded: hash rows | status words;  device only: the
    // proof-of-work bytes
    enum { CTX, HDR, UPLOADED, HASH = UPLOADED, STATUS, HOSTED, POW = HOSTED, NB };
    size_t sizes[NB] = {}, off[NB + 1];
    sizes[CTX] = sizeof(HeaderRoundCtx);
    sizes[HDR] = HEADER_BYTES * n;
    sizes[HASH] = 32 * n;
    sizes[STATUS] = 4 * n;
    sizes[POW] = n;
    const size_t total = arena_layout(sizes, off, NB);
    void *dv = nullptr, *hv = nullptr, *sv = nullptr;
    if (int e = tuple_thread_buffers(device, total, off[HOSTED], &dv, &hv, &sv)) return e;
    uint8_t* d = (uint8_t*)dv;
    uint8_t* h = (uint8_t*)hv;
    hipStream_t st = (hipStream_t)sv;

    memcpy(h + off[CTX], &r.ctx, sizeof(HeaderRoundCtx));
    host::pfor(n, 1 << 14, [&](size_t lo, size_t hi) {
        memcpy(h + off[HDR] + HEADER_BYTES * lo, r.headers + HEADER_BYTES * lo, HEADER_BYTES * (hi - lo));
    });

    EventSpans kt(g_timing, tl_ms, st);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const HeaderRoundCtx* d_ctx = (const HeaderRoundCtx*)(d + off[CTX]);
    kt.begin(HEADER_MS_UPLOAD);
    BCC_HIP_TRY(hipMemcpyAsync(d, h, off[UPLOADED], hipMemcpyHostToDevice, st));
    kt.end();
    kt.begin(HEADER_MS_HASH);
    hipLaunchKernelGGL(header_hash_kernel, grid, block, 0, st, (const uint4*)(d + off[HDR]), (uint32_t)n,
                       d_ctx, (uint4*)(d + off[HASH]), d + off[POW]);
    kt.end();
    BCC_HIP_TRY(hipGetLastError());
    kt.begin(HEADER_MS_CONTEXT);
    hipLaunchKernelGGL(header_context_kernel, grid, block, 0, st, (const uint8_t*)(d + off[HDR]),
                       (uint32_t)n, d_ctx, (const uint32_t*)(d + off[HASH]),
                       (const uint8_t*)(d + off[POW]), (int*)(d + off[STATUS]));
    kt.end();
    BCC_HIP_TRY(hipGetLastError());
    kt.begin(HEADER_MS_DOWNLOAD);
    BCC_HIP_TRY(hipMemcpyAsync(h + off[HASH], d + off[HASH], off[HOSTED] - off[HASH],
                               hipMemcpyDeviceToHost, st));
    kt.end();
    BCC_HIP_TRY(hipStreamSynchronize(st));
    kt.collect();
    host::pfor(n, 1 << 14, [&](size_t lo, size_t hi) {
        memcpy(r.hashes + 32 * lo, h + off[HASH] + 32 * lo, 32 * (hi - lo));
        memcpy(r.status + lo, h + off[STATUS] + 4 * lo, 4 * (hi - lo));
    });
    return 0;
}

int pow_round(int device, PowRound& r) {
    const size_t n = r.n;
    if (n == 0 || n > HEADER_ROUND_MAX) return (int)hipErrorInvalidValue;
    enum { HASH, BITS, UPLOADED, OK = UPLOADED, HOSTED, NB = HOSTED };
    size_t sizes[NB] = {}, off[NB + 1];
    sizes[HASH] = 32 * n;
    sizes[BITS] = 4 * n;
    sizes[OK] = n;
    const size_t total = arena_layout(sizes, off, NB);
    void *dv = nullptr, *hv = nullptr, *sv = nullptr;
    if (int e = tuple_thread_buffers(device, total, total, &dv, &hv, &sv)) return e;
    uint8_t* d = (uint8_t*)dv;
    uint8_t* h = (uint8_t*)hv;
    hipStream_t st = (hipStream_t)sv;
    memcpy(h + off[HASH], r.hash32, 32 * n);
    memcpy(h + off[BITS], r.bits, 4 * n);
    PowLimit limit;
    memcpy(limit.w, r.pow_limit, 32);
    BCC_HIP_TRY(hipMemcpyAsync(d, h, off[UPLOADED], hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pow_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       (const uint4*)(d + off[HASH]), (const uint32_t*)(d + off[BITS]), (uint32_t)n,
                       limit, d + off[OK]);
    BCC_HIP_TRY(hipGetLastError());
    BCC_HIP_TRY(hipMemcpyAsync(h + off[OK], d + off[OK], n, hipMemcpyDeviceToHost, st));
    BCC_HIP_TRY(hipStreamSynchronize(st));
    memcpy(r.ok, h + off[OK], n);
    return 0;
}

int header_round_hook(int device, HeaderRound& r) {
    const int e = header_round(device, r);
    if (e) tuple_thread_drop(device);  // wherever it failed: a re-run gets a fresh context
    return e;
}
int pow_round_hook(int device, PowRound& r) {
    const int e = pow_round(device, r);
    if (e) tuple_thread_drop(device);
    return e;
}

void header_timing_ms(double* ms, int reset) {
    for (int k = 0; k < HEADER_MS_COUNT; k++) {
        if (ms) ms[k] = tl_ms[k];
        if (reset) tl_ms[k] = 0;
    }
}

const HeaderDeviceHook header_hook{header_round_hook, pow_round_hook, header_timing_ms};
// library load: the host pass (host/headers.cpp) finds the device rounds here
const bool header_hook_set = (g_header_device_hook = &header_hook, true);

}  // namespace

}  // namespace bcc
