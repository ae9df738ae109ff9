// The host side of a device round of ECDSA-era checks (pipeline.h DeviceBatch): the parts' jobs
// and rows concatenated into a pinned image of the device arena, the upload plan, the launches of
// the sighash kernels (sighash.hip, through sighash_kernels.h) and the signature kernels
// (ecdsa_verify.hip), and the verdicts' way back; with it the gpu_verify_* / gpu_staged_* /
// gpu_early_* entry points and the page-locked pool.
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>
#include <cstring>
#include <cstdio>

#include "gpu_common.h"
#include "pipeline.h"
#include "sighash_kernels.h"
#include "host/team.h"

namespace bcc {

DeviceBatch::DeviceBatch(int device) : dev_(device) {}

// (the arenas, pinned images and shard buffers free themselves after this body, on dev_)
DeviceBatch::~DeviceBatch() {
    (void)hipSetDevice(dev_);
    if (own_stream_) (void)hipStreamDestroy((hipStream_t)own_stream_);
    if (side_stream_) (void)hipStreamDestroy((hipStream_t)side_stream_);
    if (ev_fork_) (void)hipEventDestroy((hipEvent_t)ev_fork_);
    if (ev_join_) (void)hipEventDestroy((hipEvent_t)ev_join_);
    if (ev_up_) (void)hipEventDestroy((hipEvent_t)ev_up_);
    if (ev_rows_up_) (void)hipEventDestroy((hipEvent_t)ev_rows_up_);
    if (pre_stream_) {
        (void)hipStreamSynchronize((hipStream_t)pre_stream_);
        (void)hipStreamDestroy((hipStream_t)pre_stream_);
    }
    if (ev_pre_) (void)hipEventDestroy((hipEvent_t)ev_pre_);
    if (ev_block_) (void)hipEventDestroy((hipEvent_t)ev_block_);
    if (early_stream_) {
        (void)hipStreamSynchronize((hipStream_t)early_stream_);
        (void)hipStreamDestroy((hipStream_t)early_stream_);
    }
    if (early_sig_stream_) {
        (void)hipStreamSynchronize((hipStream_t)early_sig_stream_);
        (void)hipStreamDestroy((hipStream_t)early_sig_stream_);
    }
    if (ev_early_) (void)hipEventDestroy((hipEvent_t)ev_early_);
    if (ev_early_up_) (void)hipEventDestroy((hipEvent_t)ev_early_up_);
    if (ev_early_sig_) (void)hipEventDestroy((hipEvent_t)ev_early_sig_);
}

// Early Q halves: the rows go up on the batch's early stream, then K_inv and K_keyq over them into
// early_scratch_ (their own scratch: the round's K_keyq copies from it).  The previous set's work
// (a call whose rounds never needed it) is waited for before its image and scratch are reused.
int DeviceBatch::early_launch(const TupleRows* const* Rw, size_t P, const SighashJobs* const* Jp) {
    early_n_ = 0;
    early_msgs_ = false;
    BCC_HIP_TRY(hipSetDevice(dev_));
    if (!early_stream_) {
        hipStream_t s = nullptr, s2 = nullptr;
        hipEvent_t e = nullptr, e2 = nullptr, e3 = nullptr;
        BCC_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        BCC_HIP_TRY(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
        BCC_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        BCC_HIP_TRY(hipEventCreateWithFlags(&e2, hipEventDisableTiming));
        BCC_HIP_TRY(hipEventCreateWithFlags(&e3, hipEventDisableTiming));
        early_stream_ = s;
        early_sig_stream_ = s2;
        ev_early_ = e;
        ev_early_up_ = e2;
        ev_early_sig_ = e3;
    }
    hipStream_t es = (hipStream_t)early_stream_, ss = (hipStream_t)early_sig_stream_;
    if (early_pending_) {
        BCC_HIP_TRY(hipStreamSynchronize(es));
        BCC_HIP_TRY(hipStreamSynchronize(ss));
        early_pending_ = false;
    }
    const std::vector<PartExtent> at = part_starts(Jp, Rw, P);
    bool need_y = false;
    for (size_t p = 0; p < P; p++) need_y |= !Rw[p]->y_unused && Rw[p]->size() != 0;
    const size_t R = at[P].row, NT = at[P].tjob;
    if (R == 0) return 0;
    if (at[P].tpl >= ((size_t)1 << 32) || at[P].code >= ((size_t)1 << 32)) return (int)hipErrorInvalidValue;
    // tag | x | y | r | s | TPL | CODE | TJOB (uploaded) | MSG (device-written), each 256-aligned
    enum { TAG, X, Y, RR, S, TPL, CODE, TJOB, MSG, NB };
    size_t sizes[NB] = {}, off[NB + 1];
    sizes[TAG] = R; sizes[X] = sizes[Y] = sizes[RR] = sizes[S] = 32 * R;
    sizes[TPL] = at[P].tpl + 64; sizes[CODE] = at[P].code + 64; sizes[TJOB] = sizeof(TplJob) * NT;
    sizes[MSG] = NT ? 32 * R : 0;
    const size_t total = arena_layout(sizes, off, NB), upload = NT ? off[MSG] : off[TPL];
    const size_t o_tag = off[TAG], o_x = off[X], o_y = off[Y], o_r = off[RR], o_s = off[S],
                 o_tpl = off[TPL], o_code = off[CODE], o_tj = off[TJOB], o_msg = off[MSG];
    if (int e = early_arena_.reserve(total)) return e;
    if (int e = early_host_.reserve(upload)) return e;
    uint8_t* h = early_host_.bytes();
    auto fill = [&](size_t p) {
        const TupleRows& rw = *Rw[p];
        const size_t r0 = at[p].row, nr = rw.size();
        if (!nr) return;
        memcpy(h + o_tag + r0, rw.tag.data(), nr);
        memcpy(h + o_x + 32 * r0, rw.x.data(), 32 * nr);
        if (need_y) rw.copy_y(h + o_y + 32 * r0, 0, nr);
        memcpy(h + o_r + 32 * r0, rw.r.data(), 32 * nr);
        memcpy(h + o_s + 32 * r0, rw.s.data(), 32 * nr);
        if (!NT || !Jp || !Jp[p]) return;
        const SighashJobs& j = *Jp[p];
        if (!j.tpl.empty()) memcpy(h + o_tpl + at[p].tpl, j.tpl.data(), j.tpl.size());
        if (!j.code.empty()) memcpy(h + o_code + at[p].code, j.code.data(), j.code.size());
        const PartBase base = part_base(at[p]);
        TplJob* tj = (TplJob*)(h + o_tj) + at[p].tjob;
        for (size_t k = 0; k < j.tjobs.size(); k++) {
            TplJob t = j.tjobs[k];
            rebase(t, base);
            t.nblk &= ~TPL_EARLY;
            tj[k] = t;
        }
    };
    if (NT) {  // the blobs' tails the lanes may read past (dword loads)
        memset(h + o_tpl + at[P].tpl, 0, 64);
        memset(h + o_code + at[P].code, 0, 64);
    }
    if (P > 1 && R >= 4096) host::run_team((unsigned)std::min<size_t>(P, 16), [&](unsigned t) {
        for (size_t p = t; p < P; p += std::min<size_t>(P, 16)) fill(p);
    });
    else
        for (size_t p = 0; p < P; p++) fill(p);
    uint8_t* a = early_arena_.bytes();
    BCC_HIP_TRY(hipMemcpyAsync(a, h, need_y ? upload : o_y, hipMemcpyHostToDevice, es));
    if (!need_y) BCC_HIP_TRY(hipMemcpyAsync(a + o_r, h + o_r, upload - o_r, hipMemcpyHostToDevice, es));
    if (NT) {  // the early sighashes on their own stream, beside K_inv / K_keyq
        BCC_HIP_TRY(hipEventRecord((hipEvent_t)ev_early_up_, es));
        BCC_HIP_TRY(hipStreamWaitEvent(ss, (hipEvent_t)ev_early_up_, 0));
        hipLaunchKernelGGL(sighash_front_kernel, dim3((unsigned)((NT + XS_WG - 1) / XS_WG)), dim3(XS_WG), 0,
                           ss, nullptr, nullptr, 0u, nullptr, nullptr, a + o_tpl, a + o_code,
                           (const TplJob*)(a + o_tj), (uint32_t)NT, nullptr, nullptr, nullptr, 0u,
                           nullptr, a + o_msg);
        BCC_HIP_TRY(hipGetLastError());
        BCC_HIP_TRY(hipEventRecord((hipEvent_t)ev_early_sig_, ss));
        early_msg_ = a + o_msg;
    }
    const uint8_t *dt = a + o_tag, *dx = a + o_x, *dy = a + o_y, *dr = a + o_r, *ds = a + o_s;
    if (int e = ecdsa_launch_pre(early_scratch_, ds, R, es)) return e;
    if (int e = ecdsa_launch_q(early_scratch_, dt, dx, dy, dr, ds, R, es)) return e;
    const bool launched = early_scratch_.q_ready == R;
    early_scratch_.q_ready = 0;
    BCC_HIP_TRY(hipEventRecord((hipEvent_t)ev_early_, es));
    early_pending_ = true;
    if (launched) {
        early_n_ = R;
        early_msgs_ = NT != 0;
    }
    return 0;
}

void DeviceBatch::early_reset() {
    early_n_ = 0;
    early_msgs_ = false;
}

void* DeviceBatch::pick(void* stream) {
    if (!stream) {
        if (!own_stream_) {
            hipStream_t s = nullptr;
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
            own_stream_ = s;
        }
        stream = own_stream_;
    }
    last_stream_ = stream;
    return stream;
}

// Host waits on a blocking-sync event: the waiting thread sleeps instead of spinning on a core
// (the host pass may be running beside it on the same CPU share).
int DeviceBatch::wait(void* stream) {
    if (!ev_block_) {
        hipEvent_t e = nullptr;
        BCC_HIP_TRY(hipEventCreateWithFlags(&e, hipEventBlockingSync | hipEventDisableTiming));
        ev_block_ = e;
    }
    BCC_HIP_TRY(hipEventRecord((hipEvent_t)ev_block_, (hipStream_t)stream));
    BCC_HIP_TRY(hipEventSynchronize((hipEvent_t)ev_block_));
    return 0;
}

int DeviceBatch::sync() {
    BCC_HIP_TRY(hipSetDevice(dev_));
    if (last_stream_) return wait(last_stream_);
    return 0;
}

thread_local unsigned tl_stage_threads = 0;
void set_stage_threads(unsigned n) { tl_stage_threads = n; }

static std::atomic<bool> g_direct_upload{[] {
    const char* e = getenv("BCC_DIRECT_UPLOAD");
    return !(e && atoi(e) == 0);
}()};
void set_direct_upload(bool on) { g_direct_upload.store(on, std::memory_order_relaxed); }
bool direct_upload() { return g_direct_upload.load(std::memory_order_relaxed); }

// The page-locked pool (pipeline.h, pinned_alloc): free lists per power-of-two class from 4 KiB,
// under one mutex; the pool object is never destroyed (thread-exit destructors of cached
// TupleRows may return blocks after static destruction began).  A block the runtime refused to
// pin (no device) is ordinary memory, remembered so that it is freed as such.
namespace {
struct PinPool {
    std::mutex mu;
    std::vector<void*> free_[64];
    std::vector<void*> pageable;
};
PinPool& pin_pool() {
    static PinPool* p = new PinPool;
    return *p;
}
int pin_class(size_t bytes) {
    int k = 12;
    while (((size_t)1 << k) < bytes) k++;
    return k;
}
}  // namespace
void* pinned_alloc(size_t bytes) {
    const int k = pin_class(bytes ? bytes : 1);
    PinPool& pp = pin_pool();
    {
        std::lock_guard<std::mutex> g(pp.mu);
        if (!pp.free_[k].empty()) {
            void* q = pp.free_[k].back();
            pp.free_[k].pop_back();
            return q;
        }
    }
    void* q = nullptr;
    if (hipHostMalloc(&q, (size_t)1 << k, hipHostMallocDefault) == hipSuccess && q) return q;
    (void)hipGetLastError();
    q = aligned_alloc(4096, (size_t)1 << k);
    if (!q) throw std::bad_alloc();
    std::lock_guard<std::mutex> g(pp.mu);
    pp.pageable.push_back(q);
    return q;
}
void pinned_free(void* q, size_t bytes) noexcept {
    if (!q) return;
    PinPool& pp = pin_pool();
    std::lock_guard<std::mutex> g(pp.mu);
    try {
        pp.free_[pin_class(bytes ? bytes : 1)].push_back(q);
    } catch (...) {  // out of memory for the list itself: keep the block
    }
}
void pinned_trim() {
    PinPool& pp = pin_pool();
    std::lock_guard<std::mutex> g(pp.mu);
    for (auto& l : pp.free_) {
        for (void* q : l) {
            auto it = std::find(pp.pageable.begin(), pp.pageable.end(), q);
            if (it != pp.pageable.end()) {
                pp.pageable.erase(it);
                free(q);
            } else {
                (void)hipHostFree(q);
            }
        }
        l.clear();
        l.shrink_to_fit();
    }
}

int DeviceBatch::stage(const SighashJobs& j, const TupleRows& rows) {
    const SighashJobs* jp = &j;
    const TupleRows* rp = &rows;
    return stage_parts(&jp, &rp, 1);
}

// The parts (one per host interpreter thread) are concatenated in order straight into a pinned
// host image of the device arena, each part by its own thread with its records rebased (pipeline.h
// PartBase / rebase), then the image goes to HBM in one DMA copy: no merged host copy of the
// jobs and no pageable-memory staging.
int DeviceBatch::stage_parts(const SighashJobs* const* J, const TupleRows* const* Rw, size_t P,
                             bool direct_arg) {
    if (int e = sync()) return e;  // the previous run may still read the arena / the image
    n_der_ = 0;
    const std::vector<PartExtent> at = part_starts(J, Rw, P);  // at[p]: part p's start, at[P]: totals
    const PartExtent& T = at[P];
    // per part, summed by the fill below (one pass over the records, in parallel): the template
    // jobs' blocks and the BIP143 inputs' algorithmic bytes (bcc_workload_sighash_bytes)
    std::vector<size_t> part_tjblk(P, 0), part_wbytes(P, 0);
    const size_t LIM = (size_t)1 << 32;
    if (T.aux_bytes >= LIM || T.pre_bytes >= LIM || T.tpl >= LIM || T.code >= LIM ||
        T.raw >= LIM || T.row >= LIM || T.win >= LIM / 2) {
        // the job records (PatchRec, TplJob, WtxRec, WinJob, offsets) are 32-bit: refuse, never wrap
        fprintf(stderr, "[bcc] DeviceBatch::stage_parts: a job blob exceeds 4 GiB; split the round\n");
        return (int)hipErrorInvalidValue;
    }
    n_rows_ = T.row;
    n_pre_ = T.pre_idx;
    n_aux_ = T.aux_idx;
    n_patch_ = T.patch;
    pre_blocks_ = T.pre_bytes / 64;
    aux_blocks_ = T.aux_bytes / 64;
    n_tjob_ = T.tjob;
    n_wtx_ = T.wtx;
    n_wjob_ = T.wjob;
    n_ljob_ = T.ljob;
    n_win_ = T.win;
    n_hash_ = T.hrow;
    const size_t R = n_rows_;
    // regions filled from the host image first (one copy), device-written ones after them
    // Y and M go up only when some part needs them (TupleRows::y_unused / msg_one)
    enum { TAG, X, RR, S, EMAP, MMAP, AUX, PRE, AUX_OFF, AUX_NBLK, PRE_OFF, PRE_NBLK, PRE_ROW, PATCH,
           TPL, CODE, TJOB, TXRAW, WTX, WJOB, LJOB, HROW, HPROG, ZEROS, UPLOADED, Y = UPLOADED, M, V, AUXD, INTAB, TXD,
           NB };
    bool need_y = false, need_m = false, need_e = false, need_mm = false;
    for (size_t p = 0; p < P; p++) {
        need_y |= !Rw[p]->y_unused && Rw[p]->size() != 0;
        need_m |= !Rw[p]->msg_one && Rw[p]->size() != 0;
        need_e |= !Rw[p]->emap.empty();
        need_mm |= !Rw[p]->mmap.empty();
    }
    need_e = need_e && early_n_ != 0;  // early twins exist for this batch's call (early_launch)
    // early sighashes (TPL_EARLY jobs) only with live early digests; else the jobs run as usual
    need_mm = need_mm && early_n_ != 0 && early_msgs_;
    size_t sizes[NB] = {};
    sizes[TAG] = R; sizes[X] = sizes[Y] = sizes[RR] = sizes[S] = sizes[M] = 32 * R;
    sizes[EMAP] = need_e ? 4 * R : 0;
    sizes[MMAP] = need_mm ? 4 * R : 0;
    sizes[AUX] = T.aux_bytes; sizes[PRE] = T.pre_bytes;
    sizes[AUX_OFF] = sizes[AUX_NBLK] = 4 * n_aux_;
    sizes[PRE_OFF] = sizes[PRE_NBLK] = sizes[PRE_ROW] = 4 * n_pre_;
    sizes[PATCH] = sizeof(PatchRec) * n_patch_;
    sizes[TPL] = T.tpl; sizes[CODE] = T.code; sizes[TJOB] = sizeof(TplJob) * n_tjob_;
    sizes[TXRAW] = T.raw; sizes[WTX] = sizeof(WtxRec) * n_wtx_; sizes[WJOB] = sizeof(WinJob) * n_wjob_;
    sizes[LJOB] = sizeof(LinJob) * n_ljob_;
    sizes[HROW] = 4 * n_hash_; sizes[HPROG] = 20 * n_hash_;
    sizes[ZEROS] = 64;
    sizes[V] = R; sizes[AUXD] = 32 * n_aux_; sizes[INTAB] = 8 * n_win_; sizes[TXD] = 96 * n_wtx_;
    size_t off[NB + 1];
    const size_t total = arena_layout(sizes, off, NB);
    const size_t upload = off[UPLOADED], upload_ym = off[V];  // the image holds Y and M too
    if (int e = arena_.reserve(total)) return e;
    if (int e = host_image_.reserve(upload_ym)) return e;
    uint8_t* a = arena_.bytes();
    d_tag = a + off[TAG]; d_x = a + off[X]; d_y = a + off[Y]; d_r = a + off[RR]; d_s = a + off[S];
    d_m = a + off[M]; d_v = a + off[V]; d_aux_ = a + off[AUX]; d_pre_ = a + off[PRE];
    d_auxd_ = a + off[AUXD];
    d_aux_off_ = (uint32_t*)(a + off[AUX_OFF]); d_aux_nblk_ = (uint32_t*)(a + off[AUX_NBLK]);
    d_pre_off_ = (uint32_t*)(a + off[PRE_OFF]); d_pre_nblk_ = (uint32_t*)(a + off[PRE_NBLK]);
    d_pre_row_ = (uint32_t*)(a + off[PRE_ROW]); d_patch_ = (PatchRec*)(a + off[PATCH]);
    d_tpl_ = a + off[TPL]; d_code_ = a + off[CODE]; d_tjob_ = (TplJob*)(a + off[TJOB]);
    d_txraw_ = a + off[TXRAW]; d_wtx_ = (WtxRec*)(a + off[WTX]); d_wjob_ = (WinJob*)(a + off[WJOB]);
    d_ljob_ = (LinJob*)(a + off[LJOB]);
    d_hrow_ = (uint32_t*)(a + off[HROW]); d_hprog_ = a + off[HPROG];
    d_zeros_ = a + off[ZEROS]; d_intab_ = (uint32_t*)(a + off[INTAB]); d_txd_ = a + off[TXD];
    d_emap_ = need_e ? (uint32_t*)(a + off[EMAP]) : nullptr;
    d_mmap_ = need_mm ? (uint32_t*)(a + off[MMAP]) : nullptr;
    uint8_t* h = host_image_.bytes();
    memset(h + off[ZEROS], 0, 64);
    // Per array, direct upload from the parts' page-locked arrays only in rounds of at least 64k
    // rows and when the array's pieces are large:
    // each piece is its own copy, and a copy costs a few microseconds on the issuing thread, while
    // the team fills the image at several GB/s per thread (a 13k-input C3 round and the 65,536-check
    // Taproot rounds measured slower direct, 1M C2 inputs faster: profiles/r06/ab/dropin_direct_*,
    // c3_direct_upload.txt).  Small arrays go through the image, uploaded as one span.
    constexpr size_t DIRECT_MIN_PIECE = (size_t)256 << 10, DIRECT_MIN_ROWS = 65536;
    bool dm[NB] = {};
    if (direct_arg && direct_upload() && P && R >= DIRECT_MIN_ROWS) {
        for (int b : {TAG, X, RR, S, AUX, PRE, TPL, CODE, TXRAW, HPROG})
            dm[b] = sizes[b] / P >= DIRECT_MIN_PIECE;
    }
    // the rows the host pass pre-uploaded per shard (pre_upload): gathered in the run, not sent
    bool gathered = direct_arg && pre_armed_ && pre_P_ == P && R < ((size_t)1 << 32);
    for (size_t p = 0; gathered && p < P; p++) gathered = pre_rows_[p] == Rw[p]->size();
    pre_armed_ = false;
    gather_pending_ = gathered;
    if (gathered) {
        gather_row0_.resize(P + 1);
        for (size_t p = 0; p <= P; p++) gather_row0_[p] = at[p].row;
        for (int b : {TAG, X, RR, S}) dm[b] = true;  // neither filled into the image nor uploaded
    }
    // the rows of part p in [lo, hi): the bulk of a tuple batch, copied in blocks by the team
    auto fill_rows = [&](size_t p, size_t lo, size_t hi) {
        const TupleRows& rw = *Rw[p];
        const size_t r0 = at[p].row + lo, nr = hi - lo;
        auto cp = [&](int b, size_t pos, const void* src, size_t len) {
            if (len) memcpy(h + off[b] + pos, src, len);
        };
        if (!dm[TAG]) cp(TAG, r0, rw.tag.data() + lo, nr);
        if (!dm[X]) cp(X, 32 * r0, rw.x.data() + 32 * lo, 32 * nr);
        if (!dm[RR]) cp(RR, 32 * r0, rw.r.data() + 32 * lo, 32 * nr);
        if (!dm[S]) cp(S, 32 * r0, rw.s.data() + 32 * lo, 32 * nr);
        if (need_y && nr) rw.copy_y(h + off[Y] + 32 * r0, lo, hi);  // past the stored prefix: zero
        if (need_m && nr) rw.copy_msg(h + off[M] + 32 * r0, lo, hi);  // past the stored prefix: ONE
        if (need_e && nr) rw.copy_emap((uint32_t*)(h + off[EMAP]) + r0, lo, hi);
        if (need_mm && nr) rw.copy_mmap((uint32_t*)(h + off[MMAP]) + r0, lo, hi);
    };
    // part p's jobs and key-hash records, rebased for the concatenation
    auto fill = [&](size_t p) {
        const SighashJobs& j = *J[p];
        const TupleRows& rw = *Rw[p];
        const PartExtent& s = at[p];
        const PartBase base = part_base(s);
        auto cp = [&](int b, size_t pos, const void* src, size_t len) {
            if (len) memcpy(h + off[b] + pos, src, len);
        };
        auto u32s = [&](int b, size_t idx) { return (uint32_t*)(h + off[b]) + idx; };
        if (!dm[AUX]) cp(AUX, s.aux_bytes, j.aux.data(), j.aux.size());
        if (!dm[PRE]) cp(PRE, s.pre_bytes, j.pre.data(), j.pre.size());
        if (!dm[TPL]) cp(TPL, s.tpl, j.tpl.data(), j.tpl.size());
        if (!dm[CODE]) cp(CODE, s.code, j.code.data(), j.code.size());
        if (!dm[TXRAW]) cp(TXRAW, s.raw, j.txraw.data(), j.txraw.size());
        if (!dm[HPROG]) cp(HPROG, 20 * s.hrow, rw.hprog.data(), rw.hprog.size());
        rebase_copy(u32s(AUX_OFF, s.aux_idx), j.aux_off.data(), j.aux_off.size(), base.aux_blk);
        cp(AUX_NBLK, 4 * s.aux_idx, j.aux_nblk.data(), 4 * j.aux_nblk.size());
        rebase_copy(u32s(PRE_OFF, s.pre_idx), j.pre_off.data(), j.pre_off.size(), base.pre_blk);
        rebase_copy(u32s(PRE_ROW, s.pre_idx), j.pre_row.data(), j.pre_off.size(), base.row);
        cp(PRE_NBLK, 4 * s.pre_idx, j.pre_nblk.data(), 4 * j.pre_nblk.size());
        rebase_copy((PatchRec*)(h + off[PATCH]) + s.patch, j.patches.data(), j.patches.size(), base);
        TplJob* tj = (TplJob*)(h + off[TJOB]) + s.tjob;
        size_t wb = 0, tb = 0;
        for (size_t k = 0; k < j.tjobs.size(); k++) {
            TplJob t = j.tjobs[k];
            tb += tpl_job_blocks(t);
            rebase(t, base);
            if (!need_mm) t.nblk &= ~TPL_EARLY;  // no early digests for this round: hash it here
            tj[k] = t;
        }
        WtxRec* wr = (WtxRec*)(h + off[WTX]) + s.wtx;
        for (size_t k = 0; k < j.wtx.size(); k++) {
            WtxRec t = j.wtx[k];
            wb += t.tx_len + ((t.n_in & WTX_TABLE_ONLY) ? 0 : 96);
            rebase(t, base);
            wr[k] = t;
        }
        WinJob* wj = (WinJob*)(h + off[WJOB]) + s.wjob;
        for (size_t k = 0; k < j.wjobs.size(); k++) {
            WinJob t = j.wjobs[k];
            wb += t.code_len + sizeof(WinJob) + 32;
            rebase(t, base);
            wj[k] = t;
        }
        LinJob* lj = (LinJob*)(h + off[LJOB]) + s.ljob;
        for (size_t k = 0; k < j.ljobs.size(); k++) {
            LinJob t = j.ljobs[k];
            wb += t.code_len + sizeof(LinJob) + 32;
            rebase(t, base);
            lj[k] = t;
        }
        rebase_copy(u32s(HROW, s.hrow), rw.hrow.data(), rw.hrow.size(), base.row);
        part_tjblk[p] = tb;
        part_wbytes[p] = wb;
    };
    // work items: blocks of <= 64k rows of every part, then every part's jobs
    struct Work {
        size_t p, lo, hi;  // hi == 0: part p's jobs
    };
    std::vector<Work> work;
    constexpr size_t RB = (size_t)1 << 16;
    if (!dm[TAG] || !dm[X] || !dm[RR] || !dm[S] || need_y || need_m || need_e || need_mm)
        for (size_t p = 0; p < P; p++)
            for (size_t lo = 0, nr = Rw[p]->size(); lo < nr; lo += RB)
                work.push_back(Work{p, lo, std::min(nr, lo + RB)});
    for (size_t p = 0; p < P; p++) work.push_back(Work{p, 0, 0});
    auto run_work = [&](const Work& w) {
        if (w.hi) fill_rows(w.p, w.lo, w.hi);
        else fill(w.p);
    };
    const size_t want = tl_stage_threads ? tl_stage_threads : std::max<size_t>(P, 16);
    const size_t nth = std::min(work.size(), want);
    if (nth <= 1 || upload < ((size_t)1 << 20)) {
        for (const Work& w : work) run_work(w);
    } else {
        host::run_team((unsigned)nth, [&](unsigned t) {
            for (size_t k = t; k < work.size(); k += nth) run_work(work[k]);
        });
    }
    tjob_blocks_ = 0;
    sighash_bytes_ = 0;
    for (size_t p = 0; p < P; p++) {
        tjob_blocks_ += part_tjblk[p];
        sighash_bytes_ += part_wbytes[p];
    }
    sighash_bytes_ += 64 * (pre_blocks_ + aux_blocks_ + tjob_blocks_) + 32 * (n_pre_ + n_aux_ + n_tjob_);
    BCC_HIP_TRY(hipSetDevice(dev_));
    // the copy is issued by the next run, in two parts on the two streams that need them first
    // (upload_on): the tuple rows on the side stream ahead of K_inv / K_tkey / the Q ladder, the
    // sighash inputs on the main stream ahead of the front kernel
    up_pending_ = true;
    up_copies_.clear();
    // The tuple rows first, then the sighash inputs: the copies of all streams leave in issue order
    // (one copy queue), and K_inv / K_keyq -- the round's long pole -- wait only for the rows
    // (round 6: issued part by part, rows and sighash inputs interleaved, the rows of a 500k-input
    // round landed 2.4 instead of ~1 ms after the upload began).  Each class: the image's spans (runs
    // of arrays not uploaded directly), then each part's own piece of every direct array.
    auto spans = [&](int lo, int hi) {
        for (int b = lo; b < hi;) {
            if (dm[b]) {
                b++;
                continue;
            }
            int e = b + 1;
            while (e < hi && !dm[e]) e++;
            if (off[e] > off[b]) up_copies_.push_back(UpCopy{off[b], h + off[b], off[e] - off[b], lo < AUX});
            b = e;
        }
    };
    auto piece = [&](int b, size_t pos, const void* src, size_t len) {
        if (dm[b] && len) up_copies_.push_back(UpCopy{off[b] + pos, src, len, b < AUX});
    };
    spans(0, AUX);
    for (size_t p = 0; p < P && !gathered; p++) {
        const TupleRows& rw = *Rw[p];
        const size_t nr = rw.size();
        piece(TAG, at[p].row, rw.tag.data(), nr);
        piece(X, 32 * at[p].row, rw.x.data(), 32 * nr);
        piece(RR, 32 * at[p].row, rw.r.data(), 32 * nr);
        piece(S, 32 * at[p].row, rw.s.data(), 32 * nr);
    }
    spans(AUX, UPLOADED);
    for (size_t p = 0; p < P; p++) {
        const TupleRows& rw = *Rw[p];
        const SighashJobs& j = *J[p];
        piece(AUX, at[p].aux_bytes, j.aux.data(), j.aux.size());
        piece(PRE, at[p].pre_bytes, j.pre.data(), j.pre.size());
        piece(TPL, at[p].tpl, j.tpl.data(), j.tpl.size());
        piece(CODE, at[p].code, j.code.data(), j.code.size());
        piece(TXRAW, at[p].raw, j.txraw.data(), j.txraw.size());
        piece(HPROG, 20 * at[p].hrow, rw.hprog.data(), rw.hprog.size());
    }
    if (need_y) BCC_HIP_TRY(hipMemcpy(a + off[Y], h + off[Y], 32 * R, hipMemcpyHostToDevice));
    // every row's msg is uint256 ONE (byte 0 = 1) unless a part stores its own; the sighash kernels
    // overwrite theirs.  Set with the upload, on the stream of the kernels that write the rows
    // (upload_on), so that staging never waits for the GPU.
    up_msg_one_ = !need_m && R;
    if (need_m) BCC_HIP_TRY(hipMemcpy(a + off[M], h + off[M], 32 * R, hipMemcpyHostToDevice));
    return ensure_vbuf();
}

// Raw tuples (bcc_pubkey_verify_batch from host buffers): the caller's pubkey / signature blobs,
// both offset arrays and the messages are copied as they are into the pinned image (by the team, in
// 2 MiB pieces), go up in one DMA copy, and K_der writes the rows on the device (run_ecdsa).  The
// host neither parses nor touches a row.
int DeviceBatch::stage_der(const DerTuples& t) {
    if (int e = sync()) return e;
    const size_t R = t.n;
    const uint64_t pb = t.pub_bytes(), sb = t.sig_bytes();
    n_rows_ = R;
    n_pre_ = n_aux_ = n_patch_ = pre_blocks_ = aux_blocks_ = n_tjob_ = tjob_blocks_ = 0;
    n_wtx_ = n_wjob_ = n_ljob_ = n_win_ = n_hash_ = sighash_bytes_ = 0;
    d_emap_ = nullptr;
    n_der_ = 0;
    enum { PUB, SIG, POFF, SOFF, M, UPLOADED, TAG = UPLOADED, X, Y, RR, S, V, NB };
    size_t sizes[NB] = {};
    sizes[PUB] = pb; sizes[SIG] = sb; sizes[POFF] = sizes[SOFF] = 8 * (R + 1);
    sizes[M] = sizes[X] = sizes[Y] = sizes[RR] = sizes[S] = 32 * R;
    sizes[TAG] = sizes[V] = R;
    size_t off[NB + 1];
    const size_t total = arena_layout(sizes, off, NB), upload = off[UPLOADED];
    if (int e = arena_.reserve(total)) return e;
    if (int e = host_image_.reserve(upload)) return e;
    uint8_t* a = arena_.bytes();
    d_tag = a + off[TAG]; d_x = a + off[X]; d_y = a + off[Y]; d_r = a + off[RR]; d_s = a + off[S];
    d_m = a + off[M]; d_v = a + off[V];
    d_pub_ = a + off[PUB]; d_sig_ = a + off[SIG];
    d_pub_off_ = (const uint64_t*)(a + off[POFF]); d_sig_off_ = (const uint64_t*)(a + off[SOFF]);
    uint8_t* h = host_image_.bytes();
    struct Piece {
        uint8_t* dst;
        const uint8_t* src;
        size_t len;
    };
    std::vector<Piece> work;
    constexpr size_t PIECE = (size_t)2 << 20;
    auto add = [&](int b, const void* src, size_t len) {
        for (size_t o = 0; o < len; o += PIECE)
            work.push_back(Piece{h + off[b] + o, (const uint8_t*)src + o, std::min(PIECE, len - o)});
    };
    add(PUB, t.pub_blob + t.pub_off[0], pb);
    add(SIG, t.sig_blob + t.sig_off[0], sb);
    add(POFF, t.pub_off, 8 * (R + 1));
    add(SOFF, t.sig_off, 8 * (R + 1));
    add(M, t.msg32, 32 * R);
    const size_t want = tl_stage_threads ? tl_stage_threads : 16;
    const size_t nth = std::min(work.size(), want);
    if (nth <= 1) {
        for (const Piece& w : work) memcpy(w.dst, w.src, w.len);
    } else {
        host::run_team((unsigned)nth, [&](unsigned k0) {
            for (size_t k = k0; k < work.size(); k += nth) memcpy(work[k].dst, work[k].src, work[k].len);
        });
    }
    BCC_HIP_TRY(hipSetDevice(dev_));
    up_pending_ = true;
    up_msg_one_ = false;
    up_copies_.assign(1, UpCopy{0, host_image_.p, upload, true});
    n_der_ = R;
    pub_base_ = t.pub_off[0];
    pub_bytes_ = pb;
    sig_base_ = t.sig_off[0];
    sig_bytes_ = sb;
    return ensure_vbuf();
}

// Per-shard row pre-upload (DeviceBatch::pre_arm / pre_upload).  Shard buffer layout for cap rows:
// tag at 0, then x, r, s (32 bytes a row each) from align256(cap).
static size_t pre_x_off(size_t cap) { return align256(cap); }
int DeviceBatch::pre_arm(unsigned P, size_t cap_rows) {
    pre_armed_ = false;
    gather_pending_ = false;
    if (P == 0 || P > PRE_MAX_SHARDS || cap_rows == 0) return 0;
    BCC_HIP_TRY(hipSetDevice(dev_));
    if (!pre_stream_) {
        hipStream_t st = nullptr;
        hipEvent_t e = nullptr;
        BCC_HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        BCC_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        pre_stream_ = st;
        ev_pre_ = e;
    }
    // the buffers' previous round (its gather) and pre-uploads are done before they are rewritten
    if (int e = sync()) return e;
    BCC_HIP_TRY(hipStreamSynchronize((hipStream_t)pre_stream_));
    if (cap_rows > pre_cap_ || pre_buf_.size() < P) {
        const size_t cap = std::max(cap_rows, pre_cap_);
        for (DeviceBuf& b : pre_buf_)  // every shard buffer anew, as one size
            if (int e = b.release()) return e;
        if (pre_buf_.size() < P) pre_buf_.resize(P);
        pre_cap_ = 0;
        for (DeviceBuf& b : pre_buf_)
            if (int e = b.reserve(pre_x_off(cap) + 96 * cap)) return e;
        pre_cap_ = cap;
    }
    pre_rows_.assign(P, SIZE_MAX);
    pre_P_ = P;
    pre_armed_ = true;
    return 0;
}

void DeviceBatch::pre_upload(unsigned t, const TupleRows& rw) {
    if (!pre_armed_ || t >= pre_P_) return;
    const size_t n = rw.size();
    if (n > pre_cap_) return;  // stays SIZE_MAX: this shard's rows go up with the round
    if (hipSetDevice(dev_) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    hipStream_t st = (hipStream_t)pre_stream_;
    uint8_t* b = pre_buf_[t].bytes();
    const size_t xo = pre_x_off(pre_cap_);
    bool ok = true;
    if (n) {
        ok = hipMemcpyAsync(b, rw.tag.data(), n, hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(b + xo, rw.x.data(), 32 * n, hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(b + xo + 32 * pre_cap_, rw.r.data(), 32 * n, hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(b + xo + 64 * pre_cap_, rw.s.data(), 32 * n, hipMemcpyHostToDevice, st) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        return;
    }
    pre_rows_[t] = n;  // (each worker writes its own shard's entry; read after the pass joins)
}

// The staged image's pending upload: all of it on `rows_stream` when `rest_stream` is null, else
// the tuple rows on `rows_stream` and the rest on `rest_stream`.  Stream order puts every kernel
// launched after it on the same stream behind its bytes.
int DeviceBatch::upload_on(hipStream_t rows_stream, hipStream_t rest_stream, int part) {
    if (!up_pending_) return 0;
    uint8_t* a = arena_.bytes();
    // The rows first, and the rest only after them: copies queued on two streams share the copy
    // engines, so K_inv / K_keyq would otherwise wait for most of the upload (a 500k-input round's
    // rows landed after 2.3 of its 3.6 ms of copies).  run_stages issues the rows (part 1), queues
    // the Q kernels behind them, then issues the rest (part 2): the ~50 copy calls of the rest no
    // longer hold up the Q kernels' launch.
    if (part & 1) {
        if (gather_pending_) {  // the rows the host pass already sent, into place first
            gather_pending_ = false;
            BCC_HIP_TRY(hipEventRecord((hipEvent_t)ev_pre_, (hipStream_t)pre_stream_));
            BCC_HIP_TRY(hipStreamWaitEvent(rows_stream, (hipEvent_t)ev_pre_, 0));
            RowGather g{};
            g.P = pre_P_;
            g.xoff = (uint32_t)pre_x_off(pre_cap_);
            g.cap = (uint32_t)pre_cap_;
            for (unsigned p = 0; p < pre_P_; p++) {
                g.base[p] = pre_buf_[p].bytes();
                g.row0[p] = (uint32_t)gather_row0_[p];
            }
            g.row0[pre_P_] = (uint32_t)gather_row0_[pre_P_];
            if (n_rows_) {
                hipLaunchKernelGGL(row_gather_kernel, dim3((unsigned)((n_rows_ + 255) / 256)), dim3(256), 0,
                                   rows_stream, g, (uint8_t*)d_tag, (uint4*)d_x, (uint4*)d_r, (uint4*)d_s,
                                   (uint32_t)n_rows_);
                BCC_HIP_TRY(hipGetLastError());
            }
        }
        for (const UpCopy& c : up_copies_)
            if (c.rows || !rest_stream)
                BCC_HIP_TRY(hipMemcpyAsync(a + c.dst, c.src, c.len, hipMemcpyHostToDevice, rows_stream));
        if (rest_stream) {
            if (!ev_rows_up_) {
                hipEvent_t e = nullptr;
                BCC_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                ev_rows_up_ = e;
            }
            BCC_HIP_TRY(hipEventRecord((hipEvent_t)ev_rows_up_, rows_stream));
        }
    }
    if (part & 2) {
        up_pending_ = false;
        if (rest_stream) {
            BCC_HIP_TRY(hipStreamWaitEvent(rest_stream, (hipEvent_t)ev_rows_up_, 0));
            for (const UpCopy& c : up_copies_)
                if (!c.rows)
                    BCC_HIP_TRY(hipMemcpyAsync(a + c.dst, c.src, c.len, hipMemcpyHostToDevice, rest_stream));
        }
        if (up_msg_one_) {
            up_msg_one_ = false;
            hipStream_t ms = rest_stream ? rest_stream : rows_stream;
            hipLaunchKernelGGL(msg_one_kernel, dim3((unsigned)((n_rows_ + 255) / 256)), dim3(256), 0, ms,
                               (uint4*)d_m, n_rows_);
            BCC_HIP_TRY(hipGetLastError());
        }
    }
    return 0;
}

// K_win, K_lin, K2, K3: everything of the sighash stage after K_wtx / K1 / K3'.
int DeviceBatch::launch_after_front(hipStream_t st) {
    if (n_wjob_) {  // K_win: BIP143 preimages assembled from the raw tx bytes and hashed
        hipLaunchKernelGGL(bip143_in_kernel, dim3((unsigned)((n_wjob_ + XS_WG - 1) / XS_WG)),
                           dim3(XS_WG), 0, st, d_txraw_, d_wtx_, d_wjob_, (uint32_t)n_wjob_,
                           d_intab_, d_txd_, d_code_, d_zeros_, d_m);
        BCC_HIP_TRY(hipGetLastError());
    }
    if (n_ljob_) {  // K_lin: legacy NONE / SINGLE / ANYONECANPAY preimages from the raw tx bytes
        hipLaunchKernelGGL(legacy_in_kernel, dim3((unsigned)((n_ljob_ + XS_WG - 1) / XS_WG)),
                           dim3(XS_WG), 0, st, d_txraw_, d_wtx_, d_ljob_, (uint32_t)n_ljob_,
                           d_intab_, d_code_, d_m);
        BCC_HIP_TRY(hipGetLastError());
    }
    if (n_patch_) {
        size_t th = n_patch_;
        hipLaunchKernelGGL(patch_digests_kernel, dim3((unsigned)((th + 255) / 256)), dim3(256), 0, st,
                           d_pre_, d_patch_, d_auxd_, (uint32_t)n_patch_);
        BCC_HIP_TRY(hipGetLastError());
    }
    if (n_pre_) {
        hipLaunchKernelGGL(sha256d_msgs_kernel, dim3((unsigned)((n_pre_ + 255) / 256)), dim3(256), 0, st,
                           d_pre_, d_pre_off_, d_pre_nblk_, (uint32_t)n_pre_, d_m, d_pre_row_);
        BCC_HIP_TRY(hipGetLastError());
    }
    return 0;
}

// The sighash stage with the front fused (sighash_front_kernel), then K_win, K2, K3.
int DeviceBatch::launch_front(hipStream_t st) {
    const size_t lanes = 3 * n_wtx_ + n_tjob_ + n_aux_;
    if (lanes) {
        hipLaunchKernelGGL(sighash_front_kernel, dim3((unsigned)((lanes + XS_WG - 1) / XS_WG)),
                           dim3(XS_WG), 0, st, d_txraw_, d_wtx_, (uint32_t)n_wtx_, d_intab_, d_txd_,
                           d_tpl_, d_code_, d_tjob_, (uint32_t)n_tjob_, d_aux_, d_aux_off_,
                           d_aux_nblk_, (uint32_t)n_aux_, d_auxd_, d_m);
        BCC_HIP_TRY(hipGetLastError());
    }
    return launch_after_front(st);
}

int DeviceBatch::run_sighash(void* stream) {
    BCC_HIP_TRY(hipSetDevice(dev_));
    hipStream_t st = (hipStream_t)pick(stream);
    if (!st) return (int)hipErrorOutOfMemory;
    if (int e = upload_on(st, nullptr)) return e;
    return launch_front(st);
}

int DeviceBatch::run_ecdsa(void* stream) {
    BCC_HIP_TRY(hipSetDevice(dev_));
    void* st = pick(stream);
    if (!st) return (int)hipErrorOutOfMemory;
    if (int e = upload_on((hipStream_t)st, nullptr)) return e;
    if (n_der_)  // raw tuples (stage_der): K_der writes the rows first
        if (int e = der_launch(d_pub_, d_pub_off_, pub_base_, pub_bytes_, d_sig_, d_sig_off_, sig_base_,
                               sig_bytes_, n_der_, d_tag, d_x, d_y, d_r, d_s, st))
            return e;
    if (int e = ecdsa_launch(scratch_, d_tag, d_x, d_y, d_r, d_s, d_m, d_v, n_rows_, st)) return e;
    return launch_key_hash((hipStream_t)st);  // (run() queues the verdicts; the bench times this alone)
}

// K_h160 (key_hash_kernel) over the staged key-hash conditions, after K_tfin on the same stream
// or, from run_stages, ahead of the ladder into verdicts preset to 1.
int DeviceBatch::launch_key_hash(hipStream_t st) {
    if (!n_hash_) return 0;
    hipLaunchKernelGGL(key_hash_kernel, dim3((unsigned)((n_hash_ + 255) / 256)), dim3(256), 0, st,
                       d_tag, d_x, d_y, d_hrow_, d_hprog_, (uint32_t)n_hash_, d_v);
    BCC_HIP_TRY(hipGetLastError());
    return 0;
}

int DeviceBatch::ensure_vbuf() {
    v_queued_ = false;
    // in 16s: bytes_to_host_kernel writes whole 16-byte words (cap is 0 or a multiple of 16, so
    // this grows exactly when n_rows_ > cap)
    return vbuf_.reserve_mapped((std::max<size_t>(n_rows_, 1) + 15) & ~(size_t)15);
}

int DeviceBatch::queue_verdicts(hipStream_t st) {
    v_queued_ = false;
    if (!n_rows_ || n_rows_ > vbuf_.cap || !vbuf_.dev) return 0;  // fetch_verdicts copies instead
    const uint32_t n16 = (uint32_t)((n_rows_ + 15) / 16);
    hipLaunchKernelGGL(bytes_to_host_kernel, dim3((n16 + 255) / 256), dim3(256), 0, st,
                       (const uint4*)d_v, (uint4*)vbuf_.dev, n16);
    BCC_HIP_TRY(hipGetLastError());
    v_queued_ = true;
    return 0;
}

// Calls the late fill on the host (the GPU meanwhile runs what is queued), then one H2D copy of
// the rows + digests and K_late on `st`.  The rows were range-checked against the staged batch.
int DeviceBatch::put_late(hipStream_t st, const LateMsgFill* late) {
    late_rows_.clear();
    late_digs_.clear();
    (*late)(late_rows_, late_digs_);
    const size_t k = late_rows_.size();
    if (k == 0) return 0;
    if (late_digs_.size() != 32 * k) return (int)hipErrorInvalidValue;
    for (uint32_t r : late_rows_)
        if (r >= n_rows_) return (int)hipErrorInvalidValue;
    const size_t dig_off = align256(4 * k);
    if (int e = late_host_.reserve(dig_off + 32 * k)) return e;  // (grows with k: both together)
    if (int e = late_dev_.reserve(dig_off + 32 * k)) return e;
    uint8_t* h = late_host_.bytes();
    uint8_t* d = late_dev_.bytes();
    memcpy(h, late_rows_.data(), 4 * k);
    memcpy(h + dig_off, late_digs_.data(), 32 * k);
    BCC_HIP_TRY(hipMemcpyAsync(d, h, dig_off + 32 * k, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(late_msgs_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st,
                       (const uint32_t*)d, (const uint4*)(d + dig_off), (uint32_t)k,
                       d_m);
    BCC_HIP_TRY(hipGetLastError());
    return 0;
}

// K_inv and K_key read only the s and key rows, so they run on a side stream beside the sighash
// kernels (fork / join by events: graph-capturable); prep + ladder wait for both.
int DeviceBatch::run(void* stream, const LateMsgFill* late) {
    BCC_HIP_TRY(hipSetDevice(dev_));
    hipStream_t st = (hipStream_t)pick(stream);
    if (!st) return (int)hipErrorOutOfMemory;
    if (n_rows_ == 0 || n_aux_ + n_tjob_ + n_pre_ + n_wjob_ + n_ljob_ == 0) {
        if (int e = run_sighash(st)) return e;
        if (late)
            if (int e = put_late(st, late)) return e;
        if (int e = run_ecdsa(st)) return e;  // K_h160 included
        return queue_verdicts(st);
    }
    if (int e = run_stages(st, late)) return e;
    if (!kh_done_)  // (else K_h160 ran ahead of the ladder, run_stages)
        if (int e = launch_key_hash(st)) return e;
    return queue_verdicts(st);
}

// Two streams: the sighash stage on the main stream (K_wtx + K3' + K1 fused into one front launch,
// then K_win / K2 / K3), and on the side stream everything the message does not enter: K_inv,
// then one launch with the key half of the prep, u2 and the Q ladder (ecdsa_launch_q); the G
// ladder and K_tfin wait for both.  K_h160 needs only the key rows and the programs: it runs on the
// main stream beside the Q ladder into verdicts preset to 1, and K_tfin then only clears failing
// rows (verdict_and), instead of running after K_tfin at the end of the critical path.
int DeviceBatch::run_stages(void* stream, const LateMsgFill* late) {
    hipStream_t st = (hipStream_t)stream;
    kh_done_ = false;
    if (!side_stream_) {
        hipStream_t s = nullptr;
        hipEvent_t a = nullptr, b = nullptr, c = nullptr;
        BCC_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        BCC_HIP_TRY(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        BCC_HIP_TRY(hipEventCreateWithFlags(&b, hipEventDisableTiming));
        BCC_HIP_TRY(hipEventCreateWithFlags(&c, hipEventDisableTiming));
        side_stream_ = s;
        ev_fork_ = a;
        ev_join_ = b;
        ev_up_ = c;
    }
    hipStream_t side = (hipStream_t)side_stream_;
    BCC_HIP_TRY(hipEventRecord((hipEvent_t)ev_fork_, st));
    BCC_HIP_TRY(hipStreamWaitEvent(side, (hipEvent_t)ev_fork_, 0));
    if (int e = upload_on(side, st, 1)) return e;
    BCC_HIP_TRY(hipEventRecord((hipEvent_t)ev_up_, side));  // the tuple rows are on the device
    if (int e = ecdsa_launch_pre(scratch_, d_s, n_rows_, side)) return e;
    if (d_emap_ && early_n_) {  // rows with early twins: their K_keyq results are copied
        BCC_HIP_TRY(hipStreamWaitEvent(side, (hipEvent_t)ev_early_, 0));
        if (int e = ecdsa_launch_q_mapped(scratch_, early_scratch_, early_n_, d_emap_, d_tag, d_x, d_y,
                                          d_r, d_s, n_rows_, side))
            return e;
    } else if (int e = ecdsa_launch_q(scratch_, d_tag, d_x, d_y, d_r, d_s, n_rows_, side)) {
        return e;
    }
    BCC_HIP_TRY(hipEventRecord((hipEvent_t)ev_join_, side));
    if (int e = upload_on(side, st, 2)) return e;  // the sighash inputs, behind the rows
    if (int e = launch_front(st)) return e;
    if (d_mmap_ && early_n_ && early_msgs_) {  // the early sighashes into their rows
        BCC_HIP_TRY(hipStreamWaitEvent(st, (hipEvent_t)ev_early_sig_, 0));
        BCC_HIP_TRY(hipStreamWaitEvent(st, (hipEvent_t)ev_up_, 0));  // the MMAP rows uploaded
        hipLaunchKernelGGL(early_msgs_kernel, dim3((unsigned)((n_rows_ + 255) / 256)), dim3(256), 0, st,
                           d_mmap_, (uint32_t)n_rows_, (uint32_t)early_n_, (const uint4*)early_msg_,
                           (uint4*)d_m);
        BCC_HIP_TRY(hipGetLastError());
    }
    if (n_hash_) {
        BCC_HIP_TRY(hipMemsetAsync(d_v, 1, n_rows_, st));
        BCC_HIP_TRY(hipStreamWaitEvent(st, (hipEvent_t)ev_up_, 0));  // K_h160 reads the key rows
        if (int e = launch_key_hash(st)) return e;
        kh_done_ = true;
    }
    if (late) {  // host-hashed messages: the host works while the queued kernels run
        if (!n_hash_) BCC_HIP_TRY(hipStreamWaitEvent(st, (hipEvent_t)ev_up_, 0));  // rows uploaded
        if (int e = put_late(st, late)) return e;
    }
    // (the wait for the Q launches, ev_join_, is placed by ecdsa_launch_after_pre: with a split
    // K_keyq the G ladder of the whole rounds starts before the tail round's K_keyq is done)
    return ecdsa_launch_after_pre(scratch_, d_tag, d_x, d_y, d_r, d_s, d_m, d_v, n_rows_, st,
                                  kh_done_, ev_join_);
}

// Verdicts come back through a pinned buffer of the batch (an asynchronous copy on the run's stream,
// then one host memcpy): a pageable D2H copy would pin the caller's pages on every call.
int DeviceBatch::fetch_verdicts(uint8_t* out) {
    if (!n_rows_) return sync();
    if (v_queued_) {  // written into vbuf_ by the run's last kernel
        v_queued_ = false;
        BCC_HIP_TRY(hipSetDevice(dev_));
        if (int e = wait(pick(last_stream_))) return e;
        memcpy(out, vbuf_.p, n_rows_);
        return 0;
    }
    BCC_HIP_TRY(hipSetDevice(dev_));
    if (n_rows_ > vbuf_.cap)  // (stage sized it)
        if (int e = ensure_vbuf()) return e;
    hipStream_t st = (hipStream_t)pick(last_stream_);
    BCC_HIP_TRY(hipMemcpyAsync(vbuf_.p, d_v, n_rows_, hipMemcpyDeviceToHost, st));
    if (int e = wait(st)) return e;
    memcpy(out, vbuf_.p, n_rows_);
    return 0;
}

int DeviceBatch::fetch_msgs(uint8_t* out) {
    if (up_pending_) {  // staged but never run: the rows are still the host's
        BCC_HIP_TRY(hipSetDevice(dev_));
        hipStream_t st = (hipStream_t)pick(last_stream_);
        if (int e = upload_on(st, nullptr)) return e;
    }
    if (int e = sync()) return e;
    if (n_rows_) BCC_HIP_TRY(hipMemcpy(out, d_m, 32 * n_rows_, hipMemcpyDeviceToHost));
    return 0;
}

int gpu_verify_batch(int device, const SighashJobs& jobs, const TupleRows& rows, uint8_t* verdict,
                     double* stage_seconds) {
    const SighashJobs* jp = &jobs;
    const TupleRows* rp = &rows;
    return gpu_verify_parts(device, &jp, &rp, 1, verdict, stage_seconds);
}

// one cached batch per (thread, device): repeated calls reuse the device arena, the pinned host
// image, scratch and streams, and concurrent callers never share any of them
thread_local std::vector<std::unique_ptr<DeviceBatch>> tl_batches;

static DeviceBatch* thread_batch(int device) {
    auto& cache = tl_batches;
    if (device < 0) return nullptr;
    if ((int)cache.size() <= device) cache.resize(device + 1);
    if (!cache[device]) cache[device] = std::make_unique<DeviceBatch>(device);
    return cache[device].get();
}

int gpu_early_launch(int device, const TupleRows* const* rows, size_t P, const SighashJobs* const* jobs) {
    DeviceBatch* b = thread_batch(device);
    if (!b) return (int)hipErrorInvalidDevice;
    return b->early_launch(rows, P, jobs);
}

void gpu_early_reset(int device) {
    if (device >= 0 && device < (int)tl_batches.size() && tl_batches[device]) tl_batches[device]->early_reset();
}

int gpu_verify_parts(int device, const SighashJobs* const* jobs, const TupleRows* const* rows,
                     size_t parts, uint8_t* verdict, double* stage_seconds, const LateMsgFill* late) {
    size_t n = 0;
    for (size_t p = 0; p < parts; p++) n += rows[p]->size();
    if (n == 0) return 0;
    auto& cache = tl_batches;
    if (device < 0) return (int)hipErrorInvalidDevice;
    if ((int)cache.size() <= device) cache.resize(device + 1);
    if (!cache[device]) cache[device] = std::make_unique<DeviceBatch>(device);
    DeviceBatch& b = *cache[device];
    auto t0 = std::chrono::steady_clock::now();
    int e = b.stage_parts(jobs, rows, parts, true);  // the parts outlive this synchronous round
    if (!e && stage_seconds)
        *stage_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!e) e = b.run(nullptr, late);
    if (!e) e = b.fetch_verdicts(verdict);
    if (e) cache[device].reset();  // a retry starts from a fresh batch (streams, arena, scratch)
    return e;
}

int gpu_verify_der(int device, const DerTuples& t, uint8_t* verdict) {
    if (t.n == 0) return 0;
    DeviceBatch* b = thread_batch(device);
    if (!b) return (int)hipErrorInvalidDevice;
    BCC_HIP_TRY(hipSetDevice(device));
    int e = b->stage_der(t);
    if (!e) e = b->run(nullptr, nullptr);
    if (!e) e = b->fetch_verdicts(verdict);
    if (e) tl_batches[device].reset();  // a retry starts from a fresh batch
    return e;
}

struct StagedRound {
    int dev;
    std::unique_ptr<DeviceBatch> b;
};

StagedRound* gpu_staged_new(int device) { return new StagedRound{device, nullptr}; }
void gpu_staged_free(StagedRound* s) { delete s; }

int gpu_staged_stage(StagedRound* s, const SighashJobs* const* jobs, const TupleRows* const* rows,
                     size_t parts, double* stage_seconds) {
    if (s->dev < 0) return (int)hipErrorInvalidDevice;
    BCC_HIP_TRY(hipSetDevice(s->dev));
    if (!s->b) s->b = std::make_unique<DeviceBatch>(s->dev);
    auto t0 = std::chrono::steady_clock::now();
    int e = s->b->stage_parts(jobs, rows, parts, true);  // held until gpu_staged_finish (pipeline.h)
    if (!e && stage_seconds)
        *stage_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (e) s->b.reset();
    return e;
}

int gpu_staged_stage_der(StagedRound* s, const DerTuples& t, double* stage_seconds) {
    if (s->dev < 0) return (int)hipErrorInvalidDevice;
    BCC_HIP_TRY(hipSetDevice(s->dev));
    if (!s->b) s->b = std::make_unique<DeviceBatch>(s->dev);
    auto t0 = std::chrono::steady_clock::now();
    int e = s->b->stage_der(t);
    if (!e && stage_seconds)
        *stage_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (e) s->b.reset();
    return e;
}

int gpu_staged_pre_arm(StagedRound* s, unsigned P, size_t cap_rows) {
    if (s->dev < 0) return (int)hipErrorInvalidDevice;
    BCC_HIP_TRY(hipSetDevice(s->dev));
    if (!s->b) s->b = std::make_unique<DeviceBatch>(s->dev);
    const int e = s->b->pre_arm(P, cap_rows);
    if (e) s->b.reset();
    return e;
}

void gpu_staged_pre_upload(StagedRound* s, unsigned t, const TupleRows& rows) {
    if (s->b) s->b->pre_upload(t, rows);
}

int gpu_staged_launch(StagedRound* s, const LateMsgFill* late) {
    if (!s->b) return (int)hipErrorInvalidValue;
    int e = s->b->run(nullptr, late);
    if (e) s->b.reset();
    return e;
}

int gpu_staged_finish(StagedRound* s, uint8_t* verdict) {
    if (!s->b) return (int)hipErrorInvalidValue;
    int e = s->b->fetch_verdicts(verdict);
    if (e) s->b.reset();
    return e;
}

int gpu_staged_run(StagedRound* s, uint8_t* verdict, const LateMsgFill* late) {
    if (int e = gpu_staged_launch(s, late)) return e;
    return gpu_staged_finish(s, verdict);
}


}  // namespace bcc
