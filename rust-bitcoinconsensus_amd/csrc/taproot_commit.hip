// BIP341 script-path commitment checks on the GPU: the kernels and the host half of
// bcc_taproot_commit_batch and mi_xonly_tweak_check_tuples (include/bcc_amd.h).  The lane code is
// taproot_commit.h.
//
//   K_chash  commit_hash_kernel  one lane per spend: the TapLeaf hash of its padded leaf message,
//                                one TapBranch hash per node of its control block, the TapTweak
//                                hash.  SHA-bound (two compressions per node), trip counts differ
//                                per lane (script length, depth 0..128): a wave runs as long as
//                                its deepest lane.
//   K_tadd   tweak_add_kernel    R = lift_x(p) + t G: the square root, the fixed-base comb (one
//                                table point per 16-bit window, no doublings) and one addition;
//                                decides the rows that need no comparison.  Field multiplies only,
//                                no data-dependent branches outside the rare cases.
//   K_tfin   tweak_fin_kernel    R.z^-1 by Montgomery's trick over a group of COMMIT_INV_GROUP
//                                lanes per thread (one inversion per group, as twist_fin_kernel),
//                                then x(R) == q and the parity of y(R).  A decided lane multiplies
//                                nothing into its group's product.
//   K_leaf   leaf_copy_kernel    bcc_taproot_spend_batch only: one lane per queued tapscript
//                                signature check, K_chash's TapLeaf hash of the check's spend into
//                                the check's slot of the SigMsg ext blob (HBM to HBM: the hash
//                                never visits the host).
// The host half lives here rather than under csrc/host because it launches kernels: csrc/host is
// also built into the CPU tests' device-less engine.
#include "gpu_common.h"
#include "host/devices.h"
#include "host/host_verify.h"
#include "host/taproot_host.h"
#include "host/tuples.h"
#include "pipeline.h"
#include "taproot_commit.h"
#include "taproot_spend.h"

#include <functional>

namespace bcc {

namespace {

// lanes whose R.z share one inversion (one thread of K_tfin walks lanes t, t + T, t + 2T, ...)
constexpr size_t COMMIT_INV_GROUP = 16;
// K_tfin's thread count T over a chunk of cnt lanes (curve_launch, bcc_debug_commit_fin_threads)
size_t commit_fin_threads(size_t cnt) { return (cnt + COMMIT_INV_GROUP - 1) / COMMIT_INV_GROUP; }
// K_tadd -> K_tfin scratch, word-major (word w of lane i at [w * stride + i]: coalesced):
// X, Y, Z of R, the group's running product before the lane, the lane's status
constexpr int S_X = 0, S_Y = 8, S_Z = 16, S_PRE = 24, S_STAT = 32, SCRATCH_WORDS = 33;
// lanes per K_tadd / K_tfin launch pair (bounds the scratch: 132 B per lane)
constexpr size_t CURVE_CHUNK = (size_t)1 << 20;
// items per device round of bcc_taproot_commit_batch, and the bytes of its node + leaf blobs
// (a single larger item still gets a round of its own)
constexpr size_t COMMIT_ROUND_ITEMS = (size_t)1 << 20;
constexpr size_t COMMIT_ROUND_BLOB = (size_t)512 << 20;

struct GCombGlobal {
    const u32* base;
    __device__ void get(int win, int i, fe& x, fe& y) const {
        const uint4* q = reinterpret_cast<const uint4*>(base + ((size_t)win * CTAB + i) * 16);
        const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
        x.v[0] = a.x; x.v[1] = a.y; x.v[2] = a.z; x.v[3] = a.w;
        x.v[4] = b.x; x.v[5] = b.y; x.v[6] = b.z; x.v[7] = b.w;
        y.v[0] = c.x; y.v[1] = c.y; y.v[2] = c.z; y.v[3] = c.w;
        y.v[4] = d.x; y.v[5] = d.y; y.v[6] = d.z; y.v[7] = d.w;
    }
};

// a 32-byte big-endian row (16-byte aligned) as little-endian limbs
__device__ __forceinline__ void load_row32(u32 (&v)[8], const uint8_t* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    v[7] = bswap32(a.x); v[6] = bswap32(a.y); v[5] = bswap32(a.z); v[4] = bswap32(a.w);
    v[3] = bswap32(b.x); v[2] = bswap32(b.y); v[1] = bswap32(b.z); v[0] = bswap32(b.w);
}

__device__ __forceinline__ void sw_load(u32 (&v)[8], const u32* s, size_t stride, int w0) {
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = s[(size_t)(w0 + j) * stride];
}
__device__ __forceinline__ void sw_store(u32* s, size_t stride, int w0, const u32 (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) s[(size_t)(w0 + j) * stride] = v[j];
}

__global__ __launch_bounds__(256) void commit_hash_kernel(const CommitLane* __restrict__ lanes,
                                                          const u32* __restrict__ leaf_blob,
                                                          const u32* __restrict__ node_blob,
                                                          const u32* __restrict__ p_row,
                                                          u32* __restrict__ t_row,
                                                          u32* __restrict__ leaf_row, size_t n,
                                                          CommitMids mids) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const CommitLane L = lanes[i];
    u32 leaf[8], t[8];
    if (L.depth == COMMIT_SKIP) {
#pragma unroll
        for (int j = 0; j < 8; j++) leaf[j] = t[j] = 0;
    } else {
        commit_hash_lane(mids, leaf_blob + 16 * (size_t)L.leaf_blk, L.leaf_nblk,
                         node_blob + 8 * (size_t)L.node_off, L.depth, p_row + 8 * i, leaf, t);
    }
    store_be_words(t_row + 8 * i, t);
    store_be_words(leaf_row + 8 * i, leaf);
}

__global__ __launch_bounds__(256) void tweak_add_kernel(const uint8_t* __restrict__ p_row,
                                                        const uint8_t* __restrict__ q_row,
                                                        const uint8_t* __restrict__ par_row,
                                                        const uint8_t* __restrict__ t_row,
                                                        u32* __restrict__ scratch, size_t stride,
                                                        const u32* __restrict__ gcomb, size_t cnt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    fe p, q;
    sc t;
    load_row32(p.v, p_row + 32 * i);
    load_row32(q.v, q_row + 32 * i);
    load_row32(t.v, t_row + 32 * i);
    gej R;
    GCombGlobal gc{gcomb};
    const u32 st = tweak_add_lane(p, q, par_row[i], t, gc, R);
    u32* s = scratch + i;
    s[(size_t)S_STAT * stride] = st;
    if (st != TC_NORMAL) return;
    sw_store(s, stride, S_X, R.x.v);
    sw_store(s, stride, S_Y, R.y.v);
    sw_store(s, stride, S_Z, R.z.v);
}

__global__ __launch_bounds__(256) void tweak_fin_kernel(u32* __restrict__ scratch, size_t stride,
                                                        const uint8_t* __restrict__ q_row,
                                                        const uint8_t* __restrict__ par_row,
                                                        uint8_t* __restrict__ verdict, size_t cnt,
                                                        size_t T) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T || t >= cnt) return;
    fe acc = fe_one();
    size_t last = t;
    for (size_t i = t; i < cnt; i += T) {
        u32* s = scratch + i;
        if (s[(size_t)S_STAT * stride] == TC_NORMAL) {  // a decided lane leaves the product alone
            fe z;
            sw_store(s, stride, S_PRE, acc.v);
            sw_load(z.v, s, stride, S_Z);
            fe_mul(acc, acc, z);
        }
        last = i;
    }
    fe inv;
    fe_inv(inv, acc);  // acc != 0: every factor is the z of a finite point
    for (size_t i = last + T; i > t;) {
        i -= T;
        const u32* s = scratch + i;
        const u32 st = s[(size_t)S_STAT * stride];
        int ok = st == TC_TRUE;
        if (st == TC_NORMAL) {
            fe pre, zinv, q;
            gej R;
            sw_load(pre.v, s, stride, S_PRE);
            sw_load(R.x.v, s, stride, S_X);
            sw_load(R.y.v, s, stride, S_Y);
            sw_load(R.z.v, s, stride, S_Z);
            fe_mul(zinv, inv, pre);
            fe_mul(inv, inv, R.z);
            load_row32(q.v, q_row + 32 * i);
            ok = tweak_fin_lane(R, zinv, q, par_row[i]);
        }
        verdict[i] = (uint8_t)ok;
    }
}

// Per-kernel event times of the calling thread's last entry-point call (bcc_commit_last_kernel_ms;
// only with BCC_COMMIT_TIMING=1 in the environment: the events cost a few microseconds a launch).
enum { KT_HASH = 0, KT_ADD = 1, KT_FIN = 2, KT_KERNELS = 3 };
const bool g_timing = [] {
    const char* e = getenv("BCC_COMMIT_TIMING");
    return e && atoi(e) != 0;
}();
thread_local double tl_kernel_ms[KT_KERNELS];

struct KernelTimer {
    struct Span {
        hipEvent_t a, b;
        int k;
    };
    std::vector<Span> spans;
    hipStream_t st = nullptr;
    void begin(int k) {
        if (!g_timing) return;
        Span s{nullptr, nullptr, k};
        if (hipEventCreate(&s.a) != hipSuccess || hipEventCreate(&s.b) != hipSuccess) return;
        (void)hipEventRecord(s.a, st);
        spans.push_back(s);
    }
    void end() {
        if (g_timing && !spans.empty()) (void)hipEventRecord(spans.back().b, st);
    }
    // after the stream has been synchronised
    void collect() {
        for (Span& s : spans) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) tl_kernel_ms[s.k] += ms;
        }
    }
    ~KernelTimer() {
        for (Span& s : spans) {
            (void)hipEventDestroy(s.a);
            (void)hipEventDestroy(s.b);
        }
    }
};

// K_tadd + K_tfin over n device-resident rows in chunks of `stride` lanes of scratch.
int curve_launch(const uint8_t* d_p, const uint8_t* d_q, const uint8_t* d_par, const uint8_t* d_t,
                 uint8_t* d_verdict, size_t n, u32* d_scratch, size_t stride, hipStream_t st,
                 KernelTimer& kt) {
    int dev = 0, cus = 0;
    const u32* gcomb = nullptr;
    if (int e = comb_device_tables(&dev, &gcomb, &cus)) return e;
    for (size_t base = 0; base < n; base += stride) {
        const size_t cnt = std::min(stride, n - base);
        const size_t T = commit_fin_threads(cnt);
        kt.begin(KT_ADD);
        hipLaunchKernelGGL(tweak_add_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st,
                           d_p + 32 * base, d_q + 32 * base, d_par + base, d_t + 32 * base, d_scratch,
                           stride, gcomb, cnt);
        kt.end();
        BCC_HIP_TRY(hipGetLastError());
        kt.begin(KT_FIN);
        hipLaunchKernelGGL(tweak_fin_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st,
                           d_scratch, stride, d_q + 32 * base, d_par + base, d_verdict + base, cnt, T);
        kt.end();
        BCC_HIP_TRY(hipGetLastError());
    }
    return 0;
}

size_t scratch_bytes(size_t stride) { return align256(stride * SCRATCH_WORDS * sizeof(u32)); }

const CommitMids& mids() {
    static const CommitMids m = commit_mids();
    return m;
}

GCombArray host_comb() { return GCombArray{static_cast<const fe*>(host::host_comb_tables())}; }

// ---- tuple level ---------------------------------------------------------------------------

void tuples_host(const uint8_t* q32, const uint8_t* par, const uint8_t* p32, const uint8_t* t32,
                 uint8_t* verdict, size_t n) {
    const GCombArray gc = host_comb();
    host::pfor(n, 4, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++)
            verdict[i] = (uint8_t)xonly_tweak_check_lane(q32 + 32 * i, par[i], p32 + 32 * i,
                                                         t32 + 32 * i, gc);
    });
}

// One device's share of mi_xonly_tweak_check_tuples, in rounds of CURVE_CHUNK rows: rows
// [first, first + count) (one round, or all of them with count = n).
int tuples_rounds(int device, const uint8_t* q32, const uint8_t* par, const uint8_t* p32,
                  const uint8_t* t32, uint8_t* verdict, size_t n, size_t first, size_t count) {
    const size_t R = std::min(n, CURVE_CHUNK);
    // p | q | t | parity (uploaded) | verdict (downloaded) | curve scratch (device only)
    enum { PK, Q, T, PAR, V, S, NB };
    size_t sizes[NB] = {}, off[NB + 1];
    sizes[PK] = sizes[Q] = sizes[T] = 32 * R; sizes[PAR] = sizes[V] = R; sizes[S] = scratch_bytes(R);
    const size_t total = arena_layout(sizes, off, NB);
    const size_t o_q = off[Q], o_t = off[T], o_par = off[PAR], o_v = off[V], o_s = off[S];
    void *dv = nullptr, *hv = nullptr, *sv = nullptr;
    if (int e = tuple_thread_buffers(device, total, o_s, &dv, &hv, &sv)) return e;
    uint8_t* d = (uint8_t*)dv;
    uint8_t* h = (uint8_t*)hv;
    hipStream_t st = (hipStream_t)sv;
    for (size_t lo = first; lo < first + count; lo += R) {
        const size_t m = std::min(R, first + count - lo);
        host::pfor(m, 1 << 15, [&](size_t a, size_t b) {  // into the page-locked image, on the team
            memcpy(h + 32 * a, p32 + 32 * (lo + a), 32 * (b - a));
            memcpy(h + o_q + 32 * a, q32 + 32 * (lo + a), 32 * (b - a));
            memcpy(h + o_t + 32 * a, t32 + 32 * (lo + a), 32 * (b - a));
            memcpy(h + o_par + a, par + lo + a, b - a);
        });
        KernelTimer kt;
        kt.st = st;
        int rc = 0;
        if ((rc = (int)hipMemcpyAsync(d, h, o_v, hipMemcpyHostToDevice, st)) ||
            (rc = curve_launch(d, d + o_q, d + o_par, d + o_t, d + o_v, m, (u32*)(d + o_s), R, st, kt)) ||
            (rc = (int)hipMemcpyAsync(h + o_v, d + o_v, m, hipMemcpyDeviceToHost, st)) ||
            (rc = (int)hipStreamSynchronize(st))) {
            fprintf(stderr, "[bcc] mi_xonly_tweak_check_tuples failed: %d\n", rc);
            return rc;
        }
        kt.collect();
        memcpy(verdict + lo, h + o_v, m);
    }
    return 0;
}

// The same share under the Taproot side's failure rules (host/taproot_host.h), round by round.
int tuples_device(int device, const uint8_t* q32, const uint8_t* par, const uint8_t* p32,
                  const uint8_t* t32, uint8_t* verdict, size_t n, host::TaprootCounters& counters) {
    const size_t R = std::min(n, CURVE_CHUNK);
    host::DeviceRange range;
    for (size_t lo = 0; lo < n; lo += R) {
        const size_t m = std::min(R, n - lo);
        if (int e = host::resilient_taproot_round("mi_xonly_tweak_check_tuples", device, 0, m, range,
                                                  counters, [&] {
                const int e = tuples_rounds(device, q32, par, p32, t32, verdict, n, lo, m);
                if (e) tuple_thread_drop(device);  // a re-run gets a fresh context
                return e;
            }, [&] {
                tuples_host(q32 + 32 * lo, par + lo, p32 + 32 * lo, t32 + 32 * lo, verdict + lo, m);
            }))
            return e;
    }
    return 0;
}

// ---- commitment batch ----------------------------------------------------------------------

// The calling thread's lane records (reused from call to call)
thread_local std::vector<CommitLane> tl_lanes;

void commit_host(const bcc_taproot_commit* items, size_t n, int* ret, int* serror, uint8_t* tapleaf) {
    std::vector<CommitLane>& lanes = tl_lanes;
    lanes.resize(n);
    size_t lb = 0, nd = 0;
    commit_plan(items, n, lanes.data(), &lb, &nd);
    // u32-aligned rows: p | q | nodes | leaf | parity
    std::vector<u32> buf((64 * n + 32 * nd + 64 * lb + n + 3) / 4 + 1);
    uint8_t* b = reinterpret_cast<uint8_t*>(buf.data());
    uint8_t *p = b, *q = b + 32 * n, *nodes = q + 32 * n, *leaf = nodes + 32 * nd, *par = leaf + 64 * lb;
    const GCombArray gc = host_comb();
    const CommitMids& m = mids();
    host::pfor(n, 4, [&](size_t lo, size_t hi) {
        commit_fill(items, lanes.data(), lo, hi, p, q, par, nodes, leaf);
        for (size_t i = lo; i < hi; i++)
            commit_host_lane(m, lanes.data(), i, p, q, par, nodes, leaf, gc, ret + i, serror + i,
                             tapleaf ? tapleaf + 32 * i : nullptr);
    });
}

// One device round: items [0, n) with the blob sizes the caller's cut guarantees.
int commit_round(int device, const bcc_taproot_commit* items, size_t n, int* ret, int* serror,
                 uint8_t* tapleaf) {
    std::vector<CommitLane>& lanes = tl_lanes;
    lanes.resize(n);
    size_t lb = 0, nd = 0;
    commit_plan(items, n, lanes.data(), &lb, &nd);
    // uploaded: lanes | p | q | parity | nodes | leaf;  device only: t, then downloaded: verdict | leaf hashes
    const size_t stride = std::min(n, CURVE_CHUNK);
    enum { LANES, PK, Q, PAR, NODES, LEAF, UPLOADED, V = UPLOADED, LH, HOSTED, T = HOSTED, S, NB };
    size_t sizes[NB] = {}, off[NB + 1];
    sizes[LANES] = sizeof(CommitLane) * n; sizes[PK] = sizes[Q] = sizes[LH] = sizes[T] = 32 * n;
    sizes[PAR] = sizes[V] = n; sizes[NODES] = 32 * nd; sizes[LEAF] = 64 * lb;
    sizes[S] = scratch_bytes(stride);
    const size_t total = arena_layout(sizes, off, NB);
    const size_t o_p = off[PK], o_q = off[Q], o_par = off[PAR], o_nodes = off[NODES], o_leaf = off[LEAF],
                 o_up = off[UPLOADED], o_v = off[V], o_lh = off[LH], o_host = off[HOSTED], o_t = off[T],
                 o_s = off[S];
    void *dv = nullptr, *hv = nullptr, *sv = nullptr;
    if (int e = tuple_thread_buffers(device, total, o_host, &dv, &hv, &sv))
        return e;
    uint8_t* d = (uint8_t*)dv;
    uint8_t* h = (uint8_t*)hv;
    hipStream_t st = (hipStream_t)sv;
    memcpy(h, lanes.data(), sizeof(CommitLane) * n);
    host::pfor(n, 1 << 12, [&](size_t lo, size_t hi) {
        commit_fill(items, lanes.data(), lo, hi, h + o_p, h + o_q, h + o_par, h + o_nodes, h + o_leaf);
    });
    KernelTimer kt;
    kt.st = st;
    BCC_HIP_TRY(hipMemcpyAsync(d, h, o_up, hipMemcpyHostToDevice, st));
    kt.begin(KT_HASH);
    hipLaunchKernelGGL(commit_hash_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       (const CommitLane*)d, (const u32*)(d + o_leaf), (const u32*)(d + o_nodes),
                       (const u32*)(d + o_p), (u32*)(d + o_t), (u32*)(d + o_lh), n, mids());
    kt.end();
    BCC_HIP_TRY(hipGetLastError());
    if (int e = curve_launch(d + o_p, d + o_q, d + o_par, d + o_t, d + o_v, n, (u32*)(d + o_s), stride,
                             st, kt))
        return e;
    BCC_HIP_TRY(hipMemcpyAsync(h + o_v, d + o_v, o_host - o_v, hipMemcpyDeviceToHost, st));
    BCC_HIP_TRY(hipStreamSynchronize(st));
    kt.collect();
    const uint8_t* v = h + o_v;
    host::pfor(n, 1 << 14, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) commit_result(lanes[i], v[i], ret + i, serror + i);
    });
    if (tapleaf) memcpy(tapleaf, h + o_lh, 32 * n);
    return 0;
}

// One device's contiguous share, cut into rounds by item count and blob bytes.
int commit_range(int device, const bcc_taproot_commit* items, size_t n, int* ret, int* serror,
                 uint8_t* tapleaf, host::TaprootCounters& counters) {
    if (n <= host::host_small_round()) {
        commit_host(items, n, ret, serror, tapleaf);
        counters.round(0, n, true);
        return 0;
    }
    host::DeviceRange range;
    for (size_t lo = 0; lo < n;) {
        size_t hi = lo, blob = 0;
        while (hi < n && hi - lo < COMMIT_ROUND_ITEMS) {
            size_t b = 0;
            if (commit_control_size_ok(items[hi].control_len))
                b = 64 * commit_leaf_blocks(items[hi].script_len) + items[hi].control_len;
            if (hi > lo && blob + b > COMMIT_ROUND_BLOB) break;
            blob += b;
            hi++;
        }
        uint8_t* const lh = tapleaf ? tapleaf + 32 * lo : nullptr;
        if (int e = host::resilient_taproot_round("taproot_commit_batch", device, 0, hi - lo, range,
                                                  counters, [&] {
                const int e = commit_round(device, items + lo, hi - lo, ret + lo, serror + lo, lh);
                if (e) tuple_thread_drop(device);  // a re-run gets a fresh context
                return e;
            }, [&] { commit_host(items + lo, hi - lo, ret + lo, serror + lo, lh); })) {
            fprintf(stderr, "[bcc] bcc_taproot_commit_batch failed on device %d: %d\n", device, e);
            return e;
        }
        lo = hi;
    }
    return 0;
}

// ---- whole spends (bcc_taproot_spend_batch) ------------------------------------------------

// One lane per queued check: 32 bytes from the leaf-hash row of its spend's commitment lane to
// its slot in the ext blob, with the widest stores the slot's alignment allows (a slot follows
// 32-byte entries in a 256-aligned blob, so 16-byte stores in practice; the narrower paths keep
// the kernel right for any 4- or 1-aligned layout).  Two lanes never share a slot.
__global__ __launch_bounds__(256) void leaf_copy_kernel(const u32* __restrict__ leaf_row,
                                                        const LeafCopy* __restrict__ copies,
                                                        uint8_t* __restrict__ ext, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const LeafCopy c = copies[i];
    const uint4* src = reinterpret_cast<const uint4*>(leaf_row + 8 * (size_t)c.lane);
    const uint4 d0 = src[0], d1 = src[1];
    uint8_t* dst = ext + c.ext_byte;
    if ((c.ext_byte & 15u) == 0) {
        uint4* o = reinterpret_cast<uint4*>(dst);
        o[0] = d0;
        o[1] = d1;
    } else if ((c.ext_byte & 3u) == 0) {
        const u32 w[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
        u32* o = reinterpret_cast<u32*>(dst);
#pragma unroll
        for (int k = 0; k < 8; k++) o[k] = w[k];
    } else {
        const u32 w[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
        for (int k = 0; k < 32; k++) dst[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

// The fused round: the commitment rows ride in the Taproot round's one upload
// (gpu_taproot_begin_extra), K_chash / K_tadd / K_tfin and K_leaf run on its stream ahead of the
// SigMsg kernels, and the commitment verdicts come back with the signature verdicts.
int spend_begin(int device, int slot, const SpendRound& R) {
    const size_t P = R.P;
    std::vector<size_t> c0(P + 1, 0), k0(P + 1, 0), e0(P + 1, 0);
    std::vector<const TaprootJobs*> pj(P);
    for (size_t q = 0; q < P; q++) {
        const SpendPart& S = *R.parts[q];
        c0[q + 1] = c0[q] + S.commits.size();
        k0[q + 1] = k0[q] + S.copies.size();
        e0[q + 1] = e0[q] + S.jobs.dev.ext.size();
        pj[q] = &S.jobs;
        for (const LeafCopy& c : S.copies)  // the kernel's only indices: checked before it runs
            if (c.lane >= S.commits.size() || (size_t)c.ext_byte + 32 > S.jobs.dev.ext.size())
                return (int)hipErrorInvalidValue;
    }
    const size_t n = c0[P], nk = k0[P];
    if (e0[P] >= ((size_t)1 << 32)) return (int)hipErrorInvalidValue;
    if (n == 0) return gpu_taproot_begin_extra(device, slot, pj.data(), P, nullptr);
    // one item array for commit_plan / commit_fill (40 bytes an item)
    std::vector<bcc_taproot_commit> items(n);
    for (size_t q = 0; q < P; q++)
        std::copy(R.parts[q]->commits.begin(), R.parts[q]->commits.end(), items.begin() + c0[q]);
    std::vector<CommitLane> lanes(n);
    size_t lb = 0, nd = 0;
    commit_plan(items.data(), n, lanes.data(), &lb, &nd);
    if (lb >= ((size_t)1 << 32) || nd >= ((size_t)1 << 32)) return (int)hipErrorInvalidValue;
    // uploaded: lanes | p | q | parity | nodes | leaf | copies; device only: verdict | leaf hashes |
    // t | curve scratch
    const size_t stride = std::min(n, CURVE_CHUNK);
    enum { LANES, PK, Q, PAR, NODES, LEAF, CP, NUP };
    size_t usz[NUP] = {}, uoff[NUP + 1];
    usz[LANES] = sizeof(CommitLane) * n; usz[PK] = usz[Q] = 32 * n; usz[PAR] = n;
    usz[NODES] = 32 * nd; usz[LEAF] = 64 * lb; usz[CP] = sizeof(LeafCopy) * nk;
    const size_t up = arena_layout(usz, uoff, NUP);
    const size_t o_p = uoff[PK], o_q = uoff[Q], o_par = uoff[PAR], o_nodes = uoff[NODES],
                 o_leaf = uoff[LEAF], o_cp = uoff[CP];
    enum { V, LH, T, S, NDEV };
    size_t dsz[NDEV] = {}, doff[NDEV + 1];
    dsz[V] = n; dsz[LH] = dsz[T] = 32 * n; dsz[S] = scratch_bytes(stride);
    const size_t dev_bytes = arena_layout(dsz, doff, NDEV);
    const size_t d_v = doff[V], d_lh = doff[LH], d_t = doff[T], d_s = doff[S];
    TaprootExtra X;
    X.up_bytes = up;
    X.dev_bytes = dev_bytes;
    X.out_bytes = n;
    X.fill = [&](uint8_t* h) {
        memcpy(h, lanes.data(), sizeof(CommitLane) * n);
        host::pfor(n, 1 << 12, [&](size_t lo, size_t hi) {
            commit_fill(items.data(), lanes.data(), lo, hi, h + o_p, h + o_q, h + o_par, h + o_nodes,
                        h + o_leaf);
        });
        LeafCopy* cp = reinterpret_cast<LeafCopy*>(h + o_cp);
        for (size_t q = 0; q < P; q++) {
            const SpendPart& S = *R.parts[q];
            for (size_t k = 0; k < S.copies.size(); k++)
                cp[k0[q] + k] = LeafCopy{S.copies[k].lane + (uint32_t)c0[q],
                                         S.copies[k].ext_byte + (uint32_t)e0[q]};
        }
    };
    X.launch = [&](void* stream, uint8_t* u, uint8_t* d, uint8_t* d_ext) -> int {
        hipStream_t st = (hipStream_t)stream;
        KernelTimer kt;
        kt.st = st;
        hipLaunchKernelGGL(commit_hash_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                           (const CommitLane*)u, (const u32*)(u + o_leaf), (const u32*)(u + o_nodes),
                           (const u32*)(u + o_p), (u32*)(d + d_t), (u32*)(d + d_lh), n, mids());
        BCC_HIP_TRY(hipGetLastError());
        if (int e = curve_launch(u + o_p, u + o_q, u + o_par, d + d_t, d + d_v, n, (u32*)(d + d_s),
                                 stride, st, kt))
            return e;
        if (nk) {
            hipLaunchKernelGGL(leaf_copy_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st,
                               (const u32*)(d + d_lh), (const LeafCopy*)(u + o_cp), d_ext, (uint32_t)nk);
            BCC_HIP_TRY(hipGetLastError());
        }
        return 0;
    };
    return gpu_taproot_begin_extra(device, slot, pj.data(), P, &X);
}

int spend_end(int device, int slot, uint8_t* commit_verdict, uint8_t* sig_verdict) {
    return gpu_taproot_end_extra(device, slot, sig_verdict, nullptr, commit_verdict);
}

const SpendDeviceHook spend_hook{spend_begin, spend_end};
// library load: the host pass (host/taproot_spend.cpp) finds the device round here
const bool spend_hook_set = (g_spend_device_hook = &spend_hook, true);

// Contiguous ranges of [0, n) over the configured devices (device = -1) or the one given.
int over_devices(int device, size_t n, const std::function<int(int, size_t, size_t)>& f) {
    host::ActiveCaller active;
    std::vector<int> devs = device < 0 ? host::device_list() : std::vector<int>{device};
    const size_t D = std::max<size_t>(1, std::min<size_t>(devs.size(), (n + 4095) / 4096));
    devs.resize(D);
    std::vector<std::function<int()>> jobs;
    for (size_t k = 0; k < D; k++) {
        const size_t lo = n * k / D, hi = n * (k + 1) / D;
        const int dev = devs[k];
        jobs.push_back([=, &f] { return f(dev, lo, hi); });
    }
    return host::run_on_devices(devs, jobs);
}

}  // namespace

}  // namespace bcc

using namespace bcc;

extern "C" {

int mi_xonly_tweak_check_tuples(const uint8_t* tweaked32, const uint8_t* parity,
                                const uint8_t* internal32, const uint8_t* tweak32,
                                uint8_t* verdict, size_t n, int device) {
    if (n == 0) return 0;
    if (!tweaked32 || !parity || !internal32 || !tweak32 || !verdict) return -1;
    for (double& ms : tl_kernel_ms) ms = 0;
    host::TaprootCounters counters;
    int rc = 0;
    if (n <= host::host_small_round()) {
        tuples_host(tweaked32, parity, internal32, tweak32, verdict, n);
        counters.round(0, n, true);
    } else {
        rc = over_devices(device, n, [&](int dev, size_t lo, size_t hi) {
            return tuples_device(dev, tweaked32 + 32 * lo, parity + lo, internal32 + 32 * lo,
                                 tweak32 + 32 * lo, verdict + lo, hi - lo, counters);
        });
    }
    host::taproot_stats_store(n, counters);
    return rc;
}

int bcc_taproot_commit_batch(const bcc_taproot_commit* items, size_t n, int* ret_out,
                             int* serror_out, unsigned char* tapleaf_out, int device) {
    if (n == 0) return 0;
    if (!items || !ret_out || !serror_out) return -1;
    for (size_t i = 0; i < n; i++)
        if (!items[i].control || !items[i].program32 || (!items[i].script && items[i].script_len))
            return -1;
    for (double& ms : tl_kernel_ms) ms = 0;
    host::TaprootCounters counters;
    int rc = 0;
    if (n <= host::host_small_round()) {
        commit_host(items, n, ret_out, serror_out, tapleaf_out);
        counters.round(0, n, true);
    } else {
        rc = over_devices(device, n, [&](int dev, size_t lo, size_t hi) {
            return commit_range(dev, items + lo, hi - lo, ret_out + lo, serror_out + lo,
                                tapleaf_out ? tapleaf_out + 32 * lo : nullptr, counters);
        });
    }
    host::taproot_stats_store(n, counters);
    return rc ? -1 : 0;
}

void bcc_commit_last_kernel_ms(double* ms3) {
    for (int k = 0; k < KT_KERNELS; k++) ms3[k] = tl_kernel_ms[k];
}

size_t bcc_debug_commit_fin_threads(size_t cnt) { return commit_fin_threads(cnt); }

}  // extern "C"
