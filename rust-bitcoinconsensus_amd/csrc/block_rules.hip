// A block's transaction rules on the GPU: the kernels of bcc_tx_check_batch and
// bcc_block_check_batch (include/bcc_amd.h) and their part of the block device round.  The lane
// code and the records are block_rules.h; the round itself (the upload, K_txh, the merkle levels,
// the one synchronisation) is block_hash.hip, which calls in here through
// g_block_rules_device_hook; the host pass is host/block.cpp and host/block_rules.cpp.
//
//   K_txr    tx_rules_kernel       one lane per transaction of the round's raw blob: walks inputs
//                                  and outputs in aligned dwords, counts legacy sigops, applies
//                                  CheckTransaction's value and shape rules, notes what the block
//                                  lane needs, and writes the outpoint offsets of a transaction
//                                  with two or more inputs into the input table.
//   K_txlate tx_rules_late_kernel  the records of the long transactions, which the host evaluated
//                                  with the same lane code while K_txh and K_txr ran, into their rows.
//   K_dup    dup_input_kernel      one lane per input row: linear probing with atomicCAS in a table
//                                  of at least twice the rows; an equal outpoint of the same
//                                  transaction sets the record's duplicate word.
//   K_blk    block_rules_kernel    one wave per block: strided partial sums and minima over the
//                                  block's records, a butterfly merge, lane 0 finishes (coinbase
//                                  position, the BIP34 prefix) and writes the block's one record.
#include "block_rules.h"
#include "gpu_common.h"
#include "host/tuples.h"

#include <chrono>
#include <memory>

namespace bcc {

__global__ __launch_bounds__(256) void tx_rules_kernel(const uint32_t* __restrict__ raw,
                                                       const TxHashJob* __restrict__ jobs,
                                                       const uint32_t* __restrict__ lanes, uint32_t n,
                                                       const uint32_t* __restrict__ in_base,
                                                       InRow* __restrict__ rows,
                                                       TxRuleRec* __restrict__ recs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t job = lanes[i];
    const TxHashJob j = jobs[job];
    const uint32_t base = in_base[job], cap = in_base[job + 1] - base;
    WordBytes b(raw);
    recs[job] = tx_rules_lane(b, j.off, j.len, j.wit, rows + base, cap, job);
}

__global__ __launch_bounds__(256) void tx_rules_late_kernel(const uint32_t* __restrict__ late,
                                                            const TxRuleRec* __restrict__ src, uint32_t n,
                                                            TxRuleRec* __restrict__ recs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    recs[late[i]] = src[i];
}

struct SlotCas {
    __device__ uint32_t operator()(uint32_t* p, uint32_t expect, uint32_t v) const {
        return atomicCAS(p, expect, v);
    }
};
__global__ __launch_bounds__(256) void dup_input_kernel(const uint32_t* __restrict__ raw,
                                                        const InRow* __restrict__ rows, uint32_t n_rows,
                                                        uint32_t n_jobs, uint32_t* table,
                                                        uint32_t log2_slots, TxRuleRec* recs) {
    const uint32_t me = blockIdx.x * blockDim.x + threadIdx.x;
    if (me >= n_rows) return;
    const uint32_t tx = rows[me].tx;
    if (tx >= n_jobs) return;  // a row no lane wrote
    WordBytes b(raw);
    if (dup_input_lane(b, rows, n_rows, me, table, log2_slots, SlotCas())) recs[tx].dup = 1;
}

__device__ inline uint64_t wave_xor64(uint64_t v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
    return (uint64_t)hi << 32 | lo;
}
constexpr int BLK_WAVE = 64;
__global__ __launch_bounds__(BLK_WAVE) void block_rules_kernel(const uint32_t* __restrict__ raw,
                                                               const TxHashJob* __restrict__ jobs,
                                                               const TxRuleRec* __restrict__ recs,
                                                               const BlockRuleCtx* __restrict__ ctx,
                                                               BlockRuleOut* __restrict__ out) {
    const BlockRuleCtx c = ctx[blockIdx.x];
    BlockAcc a = block_rules_partial(recs, c, threadIdx.x, BLK_WAVE);
#pragma unroll
    for (int m = BLK_WAVE / 2; m >= 1; m >>= 1) {
        BlockAcc o;
        o.sigops = wave_xor64(a.sigops, m);
        o.stripped = wave_xor64(a.stripped, m);
        o.fail = wave_xor64(a.fail, m);
        o.nonfinal = __shfl_xor(a.nonfinal, m, 64);
        o.cb_later = __shfl_xor(a.cb_later, m, 64);
        block_acc_merge(a, o);
    }
    if (threadIdx.x != 0) return;
    WordBytes b(raw);
    out[blockIdx.x] = block_rules_finish(b, a, recs[c.job0], jobs[c.job0].off, c);
}

namespace {

const bool g_timing = [] {
    const char* e = getenv("BCC_BLOCK_TIMING");
    return e && atoi(e) != 0;
}();
thread_local double tl_ms[RULES_MS_COUNT];

// What plan() works out for the round the calling thread is about to run.
struct RulesState {
    std::vector<uint32_t> lanes, late, in_base;  // the device's jobs, the host's, the device's rows
    size_t rows = 0;
    uint32_t log2_slots = 1;
    // regions: uploaded / page-locked / device only
    enum { U_CTX, U_BASE, U_LANES, U_NB };
    enum { H_LATE, H_LATEREC, H_OUT, H_RECS, H_NB };
    enum { D_RECS, D_ROWS, D_TABLE, D_NB };
    size_t uoff[U_NB + 1], hoff[H_NB + 1], doff[D_NB + 1];
    std::unique_ptr<EventSpans> kt;
};
thread_local RulesState tl_rules;

bool job_is_long(const BlockRound& r, const TxHashJob& j) {
    return r.host_blocks && txh_chain_blocks(j) > r.host_blocks;
}

struct HostClock {  // adds its lifetime to one of the calling thread's times
    int k;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~HostClock() {
        tl_ms[k] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
};

int rules_plan(const BlockRound& r, BlockRulesPlan& p) {
    HostClock clock{RULES_MS_PLAN};
    RulesState& S = tl_rules;
    const BlockRulesRound& q = *r.rules;
    S.kt.reset();
    if (!block_rules_round_ok(r, q) || r.n_jobs == 0 || r.leaves) return 1;
    const size_t n = r.n_jobs;
    S.lanes.clear();
    S.late.clear();
    S.in_base.assign(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        const bool lng = job_is_long(r, r.jobs[i]);
        (lng ? S.late : S.lanes).push_back((uint32_t)i);
        S.in_base[i + 1] = S.in_base[i] + (lng ? 0 : q.in_base[i + 1] - q.in_base[i]);
    }
    S.rows = S.in_base[n];
    S.log2_slots = dup_table_log2(S.rows);
    size_t us[RulesState::U_NB] = {sizeof(BlockRuleCtx) * q.n_blocks, 4 * (n + 1), 4 * S.lanes.size()};
    size_t hs[RulesState::H_NB] = {4 * S.late.size(), sizeof(TxRuleRec) * S.late.size(),
                                   sizeof(BlockRuleOut) * q.n_blocks, q.recs ? sizeof(TxRuleRec) * n : 0};
    size_t ds[RulesState::D_NB] = {sizeof(TxRuleRec) * n, sizeof(InRow) * S.rows,
                                   S.rows ? (size_t)4 << S.log2_slots : 0};
    p.up_bytes = arena_layout(us, S.uoff, RulesState::U_NB);
    p.host_bytes = arena_layout(hs, S.hoff, RulesState::H_NB);
    p.dev_bytes = arena_layout(ds, S.doff, RulesState::D_NB);
    return 0;
}

void rules_fill(const BlockRound& r, uint8_t* h_up) {
    HostClock clock{RULES_MS_PLAN};
    const RulesState& S = tl_rules;
    const BlockRulesRound& q = *r.rules;
    if (q.n_blocks) memcpy(h_up + S.uoff[RulesState::U_CTX], q.ctx, sizeof(BlockRuleCtx) * q.n_blocks);
    memcpy(h_up + S.uoff[RulesState::U_BASE], S.in_base.data(), 4 * S.in_base.size());
    if (!S.lanes.empty()) memcpy(h_up + S.uoff[RulesState::U_LANES], S.lanes.data(), 4 * S.lanes.size());
}

int rules_launch(const BlockRound& r, void* stream, const uint8_t* d_raw, const TxHashJob* d_jobs,
                 uint8_t* d_up, uint8_t* h_host, uint8_t* d_host, uint8_t* d_dev) {
    RulesState& S = tl_rules;
    const BlockRulesRound& q = *r.rules;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = r.n_jobs, nl = S.lanes.size(), nlate = S.late.size(), nb = q.n_blocks;
    const uint32_t* raw = (const uint32_t*)d_raw;
    TxRuleRec* d_recs = (TxRuleRec*)(d_dev + S.doff[RulesState::D_RECS]);
    InRow* d_rows = (InRow*)(d_dev + S.doff[RulesState::D_ROWS]);
    uint32_t* d_table = (uint32_t*)(d_dev + S.doff[RulesState::D_TABLE]);
    S.kt.reset(new EventSpans(g_timing, tl_ms, st));
    EventSpans& kt = *S.kt;
    if (S.rows) {  // no row is a transaction's until a lane wrote it; every slot is empty
        BCC_HIP_TRY(hipMemsetAsync(d_rows, 0xff, sizeof(InRow) * S.rows, st));
        BCC_HIP_TRY(hipMemsetAsync(d_table, 0, (size_t)4 << S.log2_slots, st));
    }
    if (nl) {
        kt.begin(RULES_MS_TX);
        hipLaunchKernelGGL(tx_rules_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, st, raw, d_jobs,
                           (const uint32_t*)(d_up + S.uoff[RulesState::U_LANES]), (uint32_t)nl,
                           (const uint32_t*)(d_up + S.uoff[RulesState::U_BASE]), d_rows, d_recs);
        kt.end();
        BCC_HIP_TRY(hipGetLastError());
    }
    if (nlate) {  // the long transactions, on the host while the kernels run
        uint32_t* li = (uint32_t*)(h_host + S.hoff[RulesState::H_LATE]);
        TxRuleRec* lr = (TxRuleRec*)(h_host + S.hoff[RulesState::H_LATEREC]);
        memcpy(li, S.late.data(), 4 * nlate);
        HostClock clock{RULES_MS_LONG};
        host::pfor(nlate, 1, [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; k++) lr[k] = host::tx_rules_job_host(r.jobs[S.late[k]], r.src[S.late[k]]);
        });
        BCC_HIP_TRY(hipMemcpyAsync(d_host + S.hoff[RulesState::H_LATE], li,
                                   S.hoff[RulesState::H_OUT] - S.hoff[RulesState::H_LATE],
                                   hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(tx_rules_late_kernel, dim3((unsigned)((nlate + 255) / 256)), dim3(256), 0, st,
                           (const uint32_t*)(d_host + S.hoff[RulesState::H_LATE]),
                           (const TxRuleRec*)(d_host + S.hoff[RulesState::H_LATEREC]), (uint32_t)nlate, d_recs);
        BCC_HIP_TRY(hipGetLastError());
    }
    if (S.rows) {
        kt.begin(RULES_MS_DUP);
        hipLaunchKernelGGL(dup_input_kernel, dim3((unsigned)((S.rows + 255) / 256)), dim3(256), 0, st, raw,
                           (const InRow*)d_rows, (uint32_t)S.rows, (uint32_t)n, d_table, S.log2_slots, d_recs);
        kt.end();
        BCC_HIP_TRY(hipGetLastError());
    }
    if (nb) {
        BlockRuleOut* d_out = (BlockRuleOut*)(d_host + S.hoff[RulesState::H_OUT]);
        kt.begin(RULES_MS_BLOCK);
        hipLaunchKernelGGL(block_rules_kernel, dim3((unsigned)nb), dim3(BLK_WAVE), 0, st, raw, d_jobs,
                           (const TxRuleRec*)d_recs, (const BlockRuleCtx*)(d_up + S.uoff[RulesState::U_CTX]),
                           d_out);
        kt.end();
        BCC_HIP_TRY(hipGetLastError());
        BCC_HIP_TRY(hipMemcpyAsync(h_host + S.hoff[RulesState::H_OUT], d_out, sizeof(BlockRuleOut) * nb,
                                   hipMemcpyDeviceToHost, st));
    }
    if (q.recs)
        BCC_HIP_TRY(hipMemcpyAsync(h_host + S.hoff[RulesState::H_RECS], d_recs, sizeof(TxRuleRec) * n,
                                   hipMemcpyDeviceToHost, st));
    return 0;
}

void rules_collect(const BlockRound& r, const uint8_t* h_host) {
    RulesState& S = tl_rules;
    const BlockRulesRound& q = *r.rules;
    if (S.kt) S.kt->collect();
    S.kt.reset();
    if (q.n_blocks) memcpy(q.out, h_host + S.hoff[RulesState::H_OUT], sizeof(BlockRuleOut) * q.n_blocks);
    if (q.recs) memcpy(q.recs, h_host + S.hoff[RulesState::H_RECS], sizeof(TxRuleRec) * r.n_jobs);
}

void rules_timing_ms(double* ms, int reset) {
    for (int k = 0; k < RULES_MS_COUNT; k++) {
        if (ms) ms[k] = tl_ms[k];
        if (reset) tl_ms[k] = 0;
    }
}

const BlockRulesDeviceHook rules_hook{rules_plan, rules_fill, rules_launch, rules_collect, rules_timing_ms};
// library load: the block round (block_hash.hip) and the host pass find the rules' device half here
const bool rules_hook_set = (g_block_rules_device_hook = &rules_hook, true);

}  // namespace

}  // namespace bcc
