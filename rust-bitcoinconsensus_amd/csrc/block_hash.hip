// Transaction hashes and merkle trees on the GPU: the kernels and the device round of
// bcc_tx_hashes_batch, bcc_merkle_root and bcc_block_commitments_batch (include/bcc_amd.h).  The
// records, the merkle lane and the level tables are block_hash.h; the host pass is host/block.cpp.
//
//   K_txh     tx_hash_kernel       one lane per digest.  The round's transactions are uploaded once,
//                                  witnesses included; a wtxid lane streams [0, len) into the
//                                  streaming SHA-256 slot of K_win / K_lin (xsha_device.h), a txid
//                                  lane of a witness transaction streams [0, 4), [6, witness
//                                  start) and [len - 4, len), a transaction without witness data
//                                  takes one lane and its wtxid row is a copy.  xs_put loads the
//                                  aligned dwords that cover a step and funnel-shifts them, so a
//                                  range may start at any byte; what decides between its word-wise
//                                  and its byte-wise store is the fill of the block buffer, which
//                                  stays a multiple of 4 up to the last four bytes of a witness
//                                  txid (xs_put_headed there).  A lane is one serial chain: a wave
//                                  runs as long as its longest transaction.
//   K_late    late_rows_kernel     the digests of the long transactions, which the host hashed while
//                                  K_txh ran, into their rows (the trees read them on the device).
//   K_merkle  merkle_level_kernel  one lane per parent node of one level, over every tree of the
//                                  round (the block's txid tree and, where the block reaches the
//                                  commitment comparison, its witness tree): SHA-256d of 64 bytes,
//                                  equal existing siblings OR the tree's mutation word.  Levels are
//                                  launched back to back on the round's stream over ping-pong
//                                  buffers; a tree's last parent goes to its root row.
// The host half lives here rather than under csrc/host because it launches kernels.
#include "block_hash.h"
#include "block_rules.h"
#include "gpu_common.h"
#include "host/hashes.h"
#include "host/tuples.h"
#include "sighash_kernels.h"
#include "xsha_device.h"

#include <chrono>

namespace bcc {

// lane = job index * 2 + kind (0: the txid lane, 1: the wtxid lane of a witness transaction)
__global__ __launch_bounds__(XS_WG) void tx_hash_kernel(const uint8_t* __restrict__ raw,
                                                        const TxHashJob* __restrict__ jobs,
                                                        const uint32_t* __restrict__ lanes, uint32_t n,
                                                        uint8_t* __restrict__ txid_rows,
                                                        uint8_t* __restrict__ wtxid_rows) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[XS_WG * XS_SLOT];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t lane = lanes[i];
    const TxHashJob j = jobs[lane >> 1];
    const uint8_t* t = raw + j.off;
    XSha h;
    xs_init(h, lds + threadIdx.x * XS_SLOT);
    if (lane & 1u) {
        xs_put(h, t, j.len);
        xs_final_d(h, wtxid_rows + 32 * (size_t)j.row);
        return;
    }
    if (j.wit) {
        xs_put(h, t, 4);
        xs_put(h, t + 6, j.wit - 6);
        xs_put_headed(h, t + j.len - 4, 4);
    } else {
        xs_put(h, t, j.len);
    }
    uint32_t e[8];
    xs_final_dw(h, e);
    const uint4 d0 = make_uint4(bswap_u32(e[0]), bswap_u32(e[1]), bswap_u32(e[2]), bswap_u32(e[3]));
    const uint4 d1 = make_uint4(bswap_u32(e[4]), bswap_u32(e[5]), bswap_u32(e[6]), bswap_u32(e[7]));
    uint4* o = reinterpret_cast<uint4*>(txid_rows + 32 * (size_t)j.row);
    o[0] = d0;
    o[1] = d1;
    if (j.flags & (TXH_W | TXH_WZERO)) {
        uint4* w = reinterpret_cast<uint4*>(wtxid_rows + 32 * (size_t)j.row);
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        if (j.flags & TXH_WZERO) {
            w[0] = z;
            w[1] = z;
        } else if (!j.wit) {
            w[0] = d0;
            w[1] = d1;
        }
    }
}

// late[k]: node row; digest k (32 bytes, 16-aligned) goes there
__global__ __launch_bounds__(256) void late_rows_kernel(const uint32_t* __restrict__ late,
                                                        const uint4* __restrict__ digests, uint32_t n,
                                                        uint4* __restrict__ rows) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t r = late[i];
    rows[2 * r] = digests[2 * (size_t)i];
    rows[2 * r + 1] = digests[2 * (size_t)i + 1];
}

__global__ __launch_bounds__(256) void merkle_level_kernel(const MerkleSeg* __restrict__ tab,
                                                           uint32_t n_tab, uint32_t lanes,
                                                           const uint32_t* in, uint32_t* out,
                                                           uint32_t* roots, uint32_t* mut) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= lanes) return;
    const MerkleLane L = merkle_lane(tab, n_tab, g, in, out, roots);
    if (merkle_lane_run(L)) atomicOr(mut + L.seg, 1u);
}

namespace {

// Event times of the calling thread since the last reset (bcc_block_last_timing_ms; only with
// BCC_BLOCK_TIMING=1 in the environment: the events cost a few microseconds each), and the host
// clock of the staging.
enum { KT_TXH = BLOCK_MS_TXH, KT_MERKLE = BLOCK_MS_MERKLE, KT_UP = BLOCK_MS_UPLOAD,
       KT_DOWN = BLOCK_MS_DOWNLOAD, KT_KERNELS = BLOCK_MS_COUNT };
const bool g_timing = [] {
    const char* e = getenv("BCC_BLOCK_TIMING");
    return e && atoi(e) != 0;
}();
thread_local double tl_kernel_ms[KT_KERNELS];

// what the calling thread keeps between rounds
struct RoundTables {
    std::vector<uint32_t> lanes, late, level, level_lanes;
    std::vector<MerkleSeg> table;
};
thread_local RoundTables tl_tables;

int block_round(int device, BlockRound& r) {
    const auto stage0 = std::chrono::steady_clock::now();
    RoundTables& T = tl_tables;
    const size_t n = r.n_jobs, rows = r.rows, NR = r.node_rows(), nseg = r.n_segs, nt = r.n_trees;
    r.long_txs = r.merkle_launches = 0;
    // every index a kernel will use, before anything is launched
    if (r.raw_bytes >= ((size_t)1 << 32) - 8 || NR >= ((size_t)1 << 31) || n >= ((size_t)1 << 30))
        return (int)hipErrorInvalidValue;
    T.lanes.clear();
    T.late.clear();
    for (size_t i = 0; i < n; i++) {
        TxHashJob j = r.jobs[i];
        if (!txh_job_ok(j, r.raw_bytes, rows)) return (int)hipErrorInvalidValue;
        if (r.host_blocks && txh_chain_blocks(j) > r.host_blocks) {  // K_late's rows instead
            T.late.push_back(j.row);
            if (j.flags & (TXH_W | TXH_WZERO)) T.late.push_back((uint32_t)(rows + j.row));
            r.long_txs++;
            continue;
        }
        T.lanes.push_back((uint32_t)(2 * i));
        if (txh_w_lane(j)) T.lanes.push_back((uint32_t)(2 * i + 1));
    }
    for (size_t s = 0; s < nseg; s++)
        if ((size_t)r.segs[s].base + r.segs[s].n_in > NR || r.segs[s].seg >= nt)
            return (int)hipErrorInvalidValue;
    if (!merkle_levels(r.segs, nseg, T.table, T.level, T.level_lanes)) return (int)hipErrorInvalidValue;
    const size_t nl = T.lanes.size(), nlate = T.late.size(), nlev = T.level_lanes.size();

    // the rules that ride on the round (block_rules.hip): their records are checked here too
    const BlockRulesDeviceHook* rules = r.rules ? g_block_rules_device_hook : nullptr;
    BlockRulesPlan rp;
    if (r.rules && (!rules || rules->plan(r, rp) != 0)) return (int)hipErrorInvalidValue;

    // uploaded: raw | jobs | lanes | tables | mutation words (zero) | the rules' records;  then,
    // uploaded behind K_txh: late rows | late digests;  downloaded with the mutation words: roots |
    // node rows;  the rules' page-locked region;  device only: the two level buffers, the rules'
    enum { RAW, JOBS, LANES, TAB, MUT, RUP, UPLOADED, LATE = UPLOADED, LATED, ROOTS, NODES, RHOST,
           HOSTED, LVA = HOSTED, LVB, RDEV, NB };
    size_t sizes[NB] = {}, off[NB + 1];
    sizes[RAW] = n ? r.raw_bytes + 4 : 0;  // (xs_put loads whole dwords)
    sizes[JOBS] = sizeof(TxHashJob) * n;
    sizes[LANES] = 4 * nl;
    sizes[TAB] = sizeof(MerkleSeg) * T.table.size();
    sizes[MUT] = 4 * nt;
    sizes[LATE] = 4 * nlate;
    sizes[LATED] = 32 * nlate;
    sizes[ROOTS] = 32 * nt;
    sizes[NODES] = 32 * NR;
    sizes[LVA] = nlev > 1 ? 32 * NR : 0;  // (the last level writes roots only)
    sizes[LVB] = nlev > 2 ? 32 * NR : 0;
    sizes[RUP] = rp.up_bytes;
    sizes[RHOST] = rp.host_bytes;
    sizes[RDEV] = rp.dev_bytes;
    const size_t total = arena_layout(sizes, off, NB);
    void *dv = nullptr, *hv = nullptr, *sv = nullptr;
    if (int e = tuple_thread_buffers(device, total, off[HOSTED], &dv, &hv, &sv)) return e;
    uint8_t* d = (uint8_t*)dv;
    uint8_t* h = (uint8_t*)hv;
    hipStream_t st = (hipStream_t)sv;

    host::pfor(n, 256, [&](size_t lo, size_t hi) {  // into the page-locked image, on the team
        for (size_t i = lo; i < hi; i++) memcpy(h + off[RAW] + r.jobs[i].off, r.src[i], r.jobs[i].len);
    });
    if (n) memset(h + off[RAW] + r.raw_bytes, 0, 4);
    if (n) memcpy(h + off[JOBS], r.jobs, sizeof(TxHashJob) * n);
    if (nl) memcpy(h + off[LANES], T.lanes.data(), 4 * nl);
    if (!T.table.empty()) memcpy(h + off[TAB], T.table.data(), sizeof(MerkleSeg) * T.table.size());
    memset(h + off[MUT], 0, 4 * nt);
    if (rules) rules->fill(r, h + off[RUP]);

    tl_kernel_ms[BLOCK_MS_STAGE] +=
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - stage0).count();

    EventSpans kt(g_timing, tl_kernel_ms, st);
    uint8_t* d_nodes = d + off[NODES];
    kt.begin(KT_UP);
    if (off[UPLOADED]) BCC_HIP_TRY(hipMemcpyAsync(d, h, off[UPLOADED], hipMemcpyHostToDevice, st));
    if (r.leaves) {
        BCC_HIP_TRY(hipMemcpyAsync(d_nodes, r.leaves, 32 * NR, hipMemcpyHostToDevice, st));
    } else {
        // a row no lane writes comes back as zeros
        BCC_HIP_TRY(hipMemsetAsync(d_nodes, 0, 32 * NR, st));
    }
    kt.end();
    if (nl) {
        kt.begin(KT_TXH);
        hipLaunchKernelGGL(tx_hash_kernel, dim3((unsigned)((nl + XS_WG - 1) / XS_WG)), dim3(XS_WG), 0, st,
                           d + off[RAW], (const TxHashJob*)(d + off[JOBS]),
                           (const uint32_t*)(d + off[LANES]), (uint32_t)nl, d_nodes, d_nodes + 32 * rows);
        kt.end();
        BCC_HIP_TRY(hipGetLastError());
    }
    if (rules) {  // behind the upload, beside K_txh; its long transactions on the host meanwhile
        if (int e = rules->launch(r, st, d + off[RAW], (const TxHashJob*)(d + off[JOBS]), d + off[RUP],
                                  h + off[RHOST], d + off[RHOST], d + off[RDEV]))
            return e;
    }
    if (nlate) {  // the long chains, on the host while K_txh runs
        uint32_t* lr = (uint32_t*)(h + off[LATE]);
        uint8_t* ld = h + off[LATED];
        memcpy(lr, T.late.data(), 4 * nlate);
        std::vector<size_t> which;
        for (size_t i = 0; i < n; i++)
            if (txh_chain_blocks(r.jobs[i]) > r.host_blocks) which.push_back(i);
        std::vector<size_t> slot(which.size() + 1, 0);
        for (size_t k = 0; k < which.size(); k++)
            slot[k + 1] = slot[k] + ((r.jobs[which[k]].flags & (TXH_W | TXH_WZERO)) ? 2 : 1);
        host::pfor(which.size(), 1, [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; k++) {
                TxHashJob j = r.jobs[which[k]];
                j.row = 0;  // its digests side by side in the late blob
                uint8_t* out = ld + 32 * slot[k];
                host::tx_hash_job_host(j, r.src[which[k]], out, out + 32);
            }
        });
        BCC_HIP_TRY(hipMemcpyAsync(d + off[LATE], h + off[LATE], off[ROOTS] - off[LATE],
                                   hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(late_rows_kernel, dim3((unsigned)((nlate + 255) / 256)), dim3(256), 0, st,
                           (const uint32_t*)(d + off[LATE]), (const uint4*)(d + off[LATED]),
                           (uint32_t)nlate, (uint4*)d_nodes);
        BCC_HIP_TRY(hipGetLastError());
    }
    for (size_t k = 0; k < nlev; k++) {
        const uint32_t* in = (const uint32_t*)(k == 0 ? d_nodes : d + off[k & 1 ? LVA : LVB]);
        uint32_t* out = (uint32_t*)(d + off[k & 1 ? LVB : LVA]);
        const uint32_t lanes = T.level_lanes[k];
        kt.begin(KT_MERKLE);
        hipLaunchKernelGGL(merkle_level_kernel, dim3((lanes + 255) / 256), dim3(256), 0, st,
                           (const MerkleSeg*)(d + off[TAB]) + T.level[k], T.level[k + 1] - T.level[k],
                           lanes, in, out, (uint32_t*)(d + off[ROOTS]), (uint32_t*)(d + off[MUT]));
        kt.end();
        BCC_HIP_TRY(hipGetLastError());
        r.merkle_launches++;
    }
    kt.begin(KT_DOWN);
    if (nseg) {
        BCC_HIP_TRY(hipMemcpyAsync(h + off[MUT], d + off[MUT], 4 * nt, hipMemcpyDeviceToHost, st));
        BCC_HIP_TRY(hipMemcpyAsync(h + off[ROOTS], d + off[ROOTS], 32 * nt, hipMemcpyDeviceToHost, st));
    }
    const size_t want = r.leaves ? 0 : 32 * rows * (r.wtxid ? 2 : 1);
    if (want) BCC_HIP_TRY(hipMemcpyAsync(h + off[NODES], d_nodes, want, hipMemcpyDeviceToHost, st));
    kt.end();
    BCC_HIP_TRY(hipStreamSynchronize(st));
    kt.collect();
    if (rules) rules->collect(r, h + off[RHOST]);
    for (size_t s = 0; s < nseg; s++) {  // (a tree no seg names keeps the caller's row)
        const size_t t = r.segs[s].seg;
        if (r.segs[s].n_in == 0) continue;
        r.mut[t] = ((const uint32_t*)(h + off[MUT]))[t];
        memcpy(r.roots + 32 * t, h + off[ROOTS] + 32 * t, 32);
    }
    if (want) {
        host::pfor(rows, 1 << 15, [&](size_t lo, size_t hi) {
            memcpy(r.txid + 32 * lo, h + off[NODES] + 32 * lo, 32 * (hi - lo));
            if (r.wtxid) memcpy(r.wtxid + 32 * lo, h + off[NODES] + 32 * (rows + lo), 32 * (hi - lo));
        });
    }
    return 0;
}

int block_round_hook(int device, BlockRound& r) {
    const int e = block_round(device, r);
    if (e) tuple_thread_drop(device);  // wherever it failed: a re-run gets a fresh context
    return e;
}

void block_timing_ms(double* ms, int reset) {
    for (int k = 0; k < KT_KERNELS; k++) {
        if (ms) ms[k] = tl_kernel_ms[k];
        if (reset) tl_kernel_ms[k] = 0;
    }
}

const BlockDeviceHook block_hook{block_round_hook, block_timing_ms};
// library load: the host pass (host/block.cpp) finds the device round here
const bool block_hook_set = (g_block_device_hook = &block_hook, true);

}  // namespace

}  // namespace bcc
