// The device round of BIP341 / BIP342 signature checks (host/taproot.cpp builds the jobs): the
// parts' TaprootJobs concatenated into a pinned image of the round's arena (pipeline.h
// taproot_fill_part), one upload, the SigMsg / aux / TapSighash kernels of sighash.hip (through
// sighash_kernels.h), an optional guest stage (TaprootExtra), the BIP340 kernels and the verdicts'
// way back, on one of TAPROOT_SLOTS contexts per (thread, device).
#include <memory>
#include <vector>
#include <cstring>
#include <cstdio>

#include "gpu_common.h"
#include "pipeline.h"
#include "sha256_device.h"
#include "sighash_kernels.h"
#include "host/hashes.h"
#include "host/team.h"

namespace bcc {

void tapsighash_midstate(uint32_t out[8]) {
    uint8_t th[32];
    host::sha256(reinterpret_cast<const uint8_t*>("TapSighash"), 10, th);
    uint32_t w[16];
    for (int k = 0; k < 16; k++) {
        const uint8_t* b = th + 4 * (k & 7);
        w[k] = (uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | b[3];
    }
    sha256_init_state(out);
    sha256_compress(out, w);
}

namespace {

// Per (thread, device) state of gpu_taproot_verify: stream, kernel scratch, device arena and its
// pinned host image, grown on demand and reused by later calls.
struct TaprootCtx {
    int dev = -1;
    hipStream_t stream = nullptr;
    size_t n = 0, off_verdict = 0, off_msg = 0;  // the round launched by gpu_taproot_begin
    size_t xout = 0;  // its guest stage's bytes behind the verdicts in vpin (16-aligned start)
    bool live = false;  // a round (rows or a guest stage) was queued and not yet ended
    SigScratch sc;
    DeviceBuf arena;
    PinnedBuf image;
    // pinned verdicts, written by a kernel queued right behind the round's kernels
    // (gpu_taproot_begin): a copy-engine D2H would sit in the one copy queue and hold up the next
    // round's upload until this round's kernels finish (measured: rounds serialised, 16.5 -> 20 ms
    // per 1M checks), and issued later it waits behind that upload instead
    PinnedBuf vpin;  // (vpin.dev: the same pages as the device sees them)
    ~TaprootCtx() {  // (the three buffers free themselves after this body, on dev)
        if (dev >= 0) (void)hipSetDevice(dev);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

}  // namespace

int gpu_taproot_verify(int device, const TaprootJobs& J, uint8_t* verdict, uint8_t* msg32_out) {
    const TaprootJobs* p = &J;
    return gpu_taproot_verify_parts(device, &p, 1, verdict, msg32_out);
}

// The parts (one per host thread) are concatenated straight into the pinned image, each part by
// its own thread with its index fix-ups (no merged host copy), then go to HBM in one DMA copy.
// Per (thread, device) TAPROOT_SLOTS contexts: the pipelined rounds of bcc_taproot_verify_batch
// rotate through them, so one round's upload runs beside the previous round's kernels while the
// host builds the next one.
thread_local std::unique_ptr<TaprootCtx> tl_taproot_ctxs[64][TAPROOT_SLOTS];

// Frees the calling thread's device batches and Taproot contexts (bcc_release_thread_state).
extern thread_local std::vector<std::unique_ptr<DeviceBatch>> tl_batches;  // device_batch.hip
void release_device_thread_state() {
    tl_batches.clear();
    for (auto& d : tl_taproot_ctxs)
        for (auto& c : d) c.reset();
}

int gpu_taproot_verify_parts(int device, const TaprootJobs* const* Jp, size_t P, uint8_t* verdict,
                             uint8_t* msg32_out) {
    if (int e = gpu_taproot_begin(device, 0, Jp, P)) return e;
    return gpu_taproot_end(device, 0, verdict, msg32_out);
}

int gpu_taproot_begin(int device, int slot, const TaprootJobs* const* Jp, size_t P) {
    return gpu_taproot_begin_extra(device, slot, Jp, P, nullptr);
}

int gpu_taproot_end(int device, int slot, uint8_t* verdict, uint8_t* msg32_out) {
    return gpu_taproot_end_extra(device, slot, verdict, msg32_out, nullptr);
}

int gpu_taproot_begin_extra(int device, int slot, const TaprootJobs* const* Jp, size_t P,
                            const TaprootExtra* X) {
    const std::vector<TapExtent> at = part_starts(Jp, P);  // at[q]: part q's start, at[P]: totals
    const TapExtent& T = at[P];
    const size_t n = T.row;
    if (device < 0 || device >= 64 || slot < 0 || slot >= TAPROOT_SLOTS) return (int)hipErrorInvalidDevice;
    if (n == 0 && !X) {
        if (tl_taproot_ctxs[device][slot]) {
            tl_taproot_ctxs[device][slot]->n = 0;
            tl_taproot_ctxs[device][slot]->live = false;
        }
        return 0;
    }
    if (T.aux_bytes >= ((size_t)1 << 32) || T.msg_bytes >= ((size_t)1 << 32) || T.raw >= ((size_t)1 << 32) ||
        T.ext >= ((size_t)1 << 32)) {
        fprintf(stderr, "[bcc] gpu_taproot_verify: a message blob exceeds 4 GiB; split the batch\n");
        return (int)hipErrorInvalidValue;
    }
    auto& slot_ctx = tl_taproot_ctxs[device][slot];
    if (!slot_ctx) {
        auto c = std::make_unique<TaprootCtx>();
        c->dev = device;
        BCC_HIP_TRY(hipSetDevice(device));
        BCC_HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        slot_ctx = std::move(c);
    }
    TaprootCtx& c = *slot_ctx;
    c.n = 0;
    c.xout = 0;
    c.live = false;
    // this slot's previous round must be done with the arena and the pinned image
    if (hipStreamSynchronize(c.stream) != hipSuccess) {
        slot_ctx.reset();
        return (int)hipErrorLaunchFailure;
    }
    BCC_HIP_TRY(hipSetDevice(device));
    const size_t naux = T.aux_idx, nmsg = T.msg_idx, npat = T.patch, nttx = T.ttx, ntj = T.tjob;
    // layout: sig64 | pk32 | msg32 | verdict | aux | msg | aux_off | aux_nblk | msg_off |
    //         msg_nblk | msg_row | patches | txraw | TtxRec | TapJob | ext | guest upload ||
    //         aux digests | input table | tx digests | guest device block (the last four not uploaded)
    enum { SIG, PK, MSG, VER, AUX, MSGB, AUX_OFF, AUX_NBLK, MSG_OFF, MSG_NBLK, MSG_ROW, PATCH, TXRAW,
           TTX, TJOB, EXT, XUP, UPLOADED, AUXD = UPLOADED, INTAB, TTXD, XDEV, NB };
    size_t sizes[NB] = {};
    sizes[SIG] = 64 * n; sizes[PK] = 32 * n; sizes[MSG] = 32 * n; sizes[VER] = n;
    sizes[AUX] = T.aux_bytes; sizes[MSGB] = T.msg_bytes; sizes[AUX_OFF] = sizes[AUX_NBLK] = 4 * naux;
    sizes[MSG_OFF] = sizes[MSG_NBLK] = sizes[MSG_ROW] = 4 * nmsg;
    sizes[PATCH] = sizeof(PatchRec) * npat; sizes[TXRAW] = T.raw + 64;
    sizes[TTX] = sizeof(TtxRec) * nttx; sizes[TJOB] = sizeof(TapJob) * ntj; sizes[EXT] = T.ext;
    sizes[AUXD] = 32 * naux; sizes[INTAB] = 16 * T.in; sizes[TTXD] = 160 * nttx;
    const size_t xout = X ? (X->out_bytes + 15) & ~(size_t)15 : 0;
    if (X) {
        sizes[XUP] = X->up_bytes;
        sizes[XDEV] = std::max(X->dev_bytes, xout);
    }
    size_t off[NB + 1];
    const size_t total = arena_layout(sizes, off, NB), upload = off[UPLOADED];
    if (int e = c.arena.reserve(total)) return e;
    if (int e = c.image.reserve(upload)) return e;
    uint8_t* h = c.image.bytes();
    if (nmsg) memset(h + off[MSG], 0, 32 * n);  // rows the host-built path leaves unhashed
    memset(h + off[TXRAW] + T.raw, 0, 64);      // a dword past the last tx for the wire walks
    auto u32s = [&](int b) { return (uint32_t*)(h + off[b]); };
    const TapImage im{h + off[SIG], h + off[PK], h + off[AUX], h + off[MSGB],
                      u32s(AUX_OFF), u32s(AUX_NBLK), u32s(MSG_OFF), u32s(MSG_NBLK), u32s(MSG_ROW),
                      (PatchRec*)(h + off[PATCH]), h + off[TXRAW], h + off[EXT],
                      (TtxRec*)(h + off[TTX]), (TapJob*)(h + off[TJOB])};
    host::run_team((unsigned)P, [&](unsigned q) { taproot_fill_part(im, *Jp[q], at[q]); });
    if (X && X->fill) X->fill(h + off[XUP]);
    uint8_t* a = c.arena.bytes();
    hipStream_t st = c.stream;
    ShaMid mid;
    tapsighash_midstate(mid.s);
    BCC_HIP_TRY(hipMemcpyAsync(a, h, upload, hipMemcpyHostToDevice, st));
    if (X && X->launch) {  // the guest stage: behind the upload, ahead of the ext blob's readers
        if (int e = X->launch((void*)st, a + off[XUP], a + off[XDEV], a + off[EXT])) {
            slot_ctx.reset();
            return e;
        }
    }
    if (nttx) {  // KT_tx, then KT_msg: the SigMsgs from the tx bytes
        hipLaunchKernelGGL(taproot_tx_kernel, dim3((unsigned)((5 * nttx + XS_WG - 1) / XS_WG)),
                           dim3(XS_WG), 0, st, a + off[TXRAW], (const TtxRec*)(a + off[TTX]),
                           (uint32_t)nttx, (uint32_t*)(a + off[INTAB]), a + off[TTXD]);
        BCC_HIP_TRY(hipGetLastError());
    }
    if (ntj) {
        hipLaunchKernelGGL(taproot_msg_kernel, dim3((unsigned)((ntj + XS_WG - 1) / XS_WG)),
                           dim3(XS_WG), 0, st, a + off[TXRAW], (const TtxRec*)(a + off[TTX]),
                           (const TapJob*)(a + off[TJOB]), (uint32_t)ntj,
                           (const uint32_t*)(a + off[INTAB]), a + off[TTXD], a + off[EXT],
                           a + off[MSG], mid);
        BCC_HIP_TRY(hipGetLastError());
    }
    if (naux) {
        hipLaunchKernelGGL(sha256_aux_kernel, dim3((unsigned)((naux + 63) / 64)), dim3(64), 0, st,
                           a + off[AUX], (const uint32_t*)(a + off[AUX_OFF]),
                           (const uint32_t*)(a + off[AUX_NBLK]), (uint32_t)naux, a + off[AUXD]);
        BCC_HIP_TRY(hipGetLastError());
    }
    if (npat) {
        hipLaunchKernelGGL(patch_digests_kernel, dim3((unsigned)((npat + 255) / 256)), dim3(256), 0,
                           st, a + off[MSGB], (const PatchRec*)(a + off[PATCH]), a + off[AUXD],
                           (uint32_t)npat);
        BCC_HIP_TRY(hipGetLastError());
    }
    if (nmsg) {
        hipLaunchKernelGGL(tapsighash_kernel, dim3((unsigned)((nmsg + 255) / 256)), dim3(256), 0, st,
                           a + off[MSGB], (const uint32_t*)(a + off[MSG_OFF]),
                           (const uint32_t*)(a + off[MSG_NBLK]), (uint32_t)nmsg, a + off[MSG],
                           (const uint32_t*)(a + off[MSG_ROW]), mid);
        BCC_HIP_TRY(hipGetLastError());
    }
    if (n) {
        if (int e = schnorr_launch(c.sc, a + off[0], a + off[2], a + off[1], a + off[3], n, st)) {
            slot_ctx.reset();
            return e;
        }
    }
    const size_t n16 = (n + 15) & ~(size_t)15;  // the guest's bytes follow the verdicts, 16-aligned
    if (int e = c.vpin.reserve_mapped(n16 + xout)) return e;
    if (n) {
        hipLaunchKernelGGL(bytes_to_host_kernel, dim3((unsigned)((n16 / 16 + 255) / 256)), dim3(256), 0, st,
                           (const uint4*)(a + off[3]), (uint4*)c.vpin.dev, (uint32_t)(n16 / 16));
        BCC_HIP_TRY(hipGetLastError());
    }
    if (xout) {
        hipLaunchKernelGGL(bytes_to_host_kernel, dim3((unsigned)((xout / 16 + 255) / 256)), dim3(256), 0, st,
                           (const uint4*)(a + off[XDEV]), (uint4*)((uint8_t*)c.vpin.dev + n16), (uint32_t)(xout / 16));
        BCC_HIP_TRY(hipGetLastError());
    }
    c.xout = X ? X->out_bytes : 0;
    c.live = true;
    c.n = n;
    c.off_verdict = off[3];
    c.off_msg = off[2];
    return 0;
}

int gpu_taproot_end_extra(int device, int slot, uint8_t* verdict, uint8_t* msg32_out,
                          uint8_t* extra_out) {
    if (device < 0 || device >= 64 || slot < 0 || slot >= TAPROOT_SLOTS) return (int)hipErrorInvalidDevice;
    auto& slot_ctx = tl_taproot_ctxs[device][slot];
    if (!slot_ctx || !slot_ctx->live) return 0;
    TaprootCtx& c = *slot_ctx;
    BCC_HIP_TRY(hipSetDevice(device));
    const uint8_t* a = c.arena.bytes();
    const size_t n = c.n, xout = c.xout;
    c.n = 0;
    c.xout = 0;
    c.live = false;
    int rc = 0;
    // the verdicts' copy was queued by gpu_taproot_begin
    if ((msg32_out && n && (rc = (int)hipMemcpyAsync(msg32_out, a + c.off_msg, 32 * n,
                                                hipMemcpyDeviceToHost, c.stream))) ||
        (rc = (int)hipStreamSynchronize(c.stream))) {
        fprintf(stderr, "[bcc] gpu_taproot_verify failed: %d\n", rc);
        slot_ctx.reset();  // a retry starts from a fresh stream / arena / scratch
        return rc;
    }
    if (n) memcpy(verdict, c.vpin.p, n);
    if (extra_out && xout) memcpy(extra_out, c.vpin.bytes() + ((n + 15) & ~(size_t)15), xout);
    return 0;
}

}  // namespace bcc
