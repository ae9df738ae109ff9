// The kernels of sighash.hip as their launchers in device_batch.hip and taproot_round.hip see them
// (private to csrc/*.hip).  A __global__ function is launched across translation units through its
// host stub; __device__ helpers are not shared this way.
#pragma once
#include <cstddef>
#include <cstdint>

#include "gpu_common.h"
#include "pipeline.h"

namespace bcc {

// A starting SHA-256 state passed by value (kernel argument: lands in SGPRs).
struct ShaMid {
    uint32_t s[8];
};

constexpr int XS_WG = 64;      // lanes per workgroup of the extraction kernels

// K_rowgather: the pre-uploaded shards' rows into the arena's tag / x / r / s, one lane per row.
struct RowGather {
    const uint8_t* base[64];
    uint32_t row0[64 + 1];
    uint32_t P;
    uint32_t xoff;  // x's offset in a shard buffer; r, s follow at + 32 cap, + 64 cap
    uint32_t cap;
};

__global__ __launch_bounds__(256) void sha256d_msgs_kernel(const uint8_t* __restrict__ buf,
                                                           const uint32_t* __restrict__ off_blk,
                                                           const uint32_t* __restrict__ nblk,
                                                           uint32_t nmsg, uint8_t* __restrict__ out,
                                                           const uint32_t* __restrict__ out_row);
__global__ __launch_bounds__(64) void sha256_aux_kernel(const uint8_t* __restrict__ buf,
                                                        const uint32_t* __restrict__ off_blk,
                                                        const uint32_t* __restrict__ nblk,
                                                        uint32_t n, uint8_t* __restrict__ out);
__global__ __launch_bounds__(256) void tapsighash_kernel(const uint8_t* __restrict__ buf,
                                                         const uint32_t* __restrict__ off_blk,
                                                         const uint32_t* __restrict__ nblk,
                                                         uint32_t n, uint8_t* __restrict__ out,
                                                         const uint32_t* __restrict__ out_row,
                                                         ShaMid mid);
__global__ __launch_bounds__(XS_WG) void sighash_front_kernel(
    const uint8_t* __restrict__ txraw, const WtxRec* __restrict__ recs, uint32_t nwtx,
    uint32_t* __restrict__ intab, uint8_t* __restrict__ txd, const uint8_t* __restrict__ tpl,
    const uint8_t* __restrict__ code, const TplJob* __restrict__ tjobs, uint32_t ntpl,
    const uint8_t* __restrict__ aux, const uint32_t* __restrict__ aux_off,
    const uint32_t* __restrict__ aux_nblk, uint32_t naux, uint8_t* __restrict__ auxd,
    uint8_t* __restrict__ msg);
__global__ __launch_bounds__(XS_WG) void bip143_in_kernel(const uint8_t* __restrict__ txraw,
                                                          const WtxRec* __restrict__ recs,
                                                          const WinJob* __restrict__ jobs,
                                                          uint32_t n, const uint32_t* __restrict__ intab,
                                                          const uint8_t* __restrict__ txd,
                                                          const uint8_t* __restrict__ code,
                                                          const uint8_t* __restrict__ zeros,
                                                          uint8_t* __restrict__ msg);
__global__ __launch_bounds__(XS_WG) void legacy_in_kernel(const uint8_t* __restrict__ txraw,
                                                          const WtxRec* __restrict__ recs,
                                                          const LinJob* __restrict__ jobs,
                                                          uint32_t n, const uint32_t* __restrict__ intab,
                                                          const uint8_t* __restrict__ code,
                                                          uint8_t* __restrict__ msg);
__global__ __launch_bounds__(XS_WG) void taproot_tx_kernel(const uint8_t* __restrict__ raw,
                                                           const TtxRec* __restrict__ recs,
                                                           uint32_t n, uint32_t* __restrict__ intab,
                                                           uint8_t* __restrict__ ttxd);
__global__ __launch_bounds__(XS_WG) void taproot_msg_kernel(const uint8_t* __restrict__ raw,
                                                            const TtxRec* __restrict__ recs,
                                                            const TapJob* __restrict__ jobs,
                                                            uint32_t n,
                                                            const uint32_t* __restrict__ intab,
                                                            const uint8_t* __restrict__ ttxd,
                                                            const uint8_t* __restrict__ ext,
                                                            uint8_t* __restrict__ msg, ShaMid mid);
__global__ __launch_bounds__(256) void patch_digests_kernel(uint8_t* __restrict__ pre,
                                                            const PatchRec* __restrict__ patches,
                                                            const uint8_t* __restrict__ auxd,
                                                            uint32_t npatch);
__global__ void __launch_bounds__(256) row_gather_kernel(RowGather g, uint8_t* __restrict__ tag,
                                                        uint4* __restrict__ x, uint4* __restrict__ r,
                                                        uint4* __restrict__ s, uint32_t R);
__global__ void __launch_bounds__(256) msg_one_kernel(uint4* __restrict__ m, size_t n);
__global__ void __launch_bounds__(256) key_hash_kernel(const uint8_t* __restrict__ tag,
                                                       const uint8_t* __restrict__ x,
                                                       const uint8_t* __restrict__ y,
                                                       const uint32_t* __restrict__ hrow,
                                                       const uint8_t* __restrict__ hprog,
                                                       uint32_t n, uint8_t* __restrict__ verdict);
__global__ void __launch_bounds__(256) bytes_to_host_kernel(const uint4* __restrict__ src,
                                                            uint4* __restrict__ dst, uint32_t n16);
__global__ void __launch_bounds__(256) early_msgs_kernel(const uint32_t* __restrict__ mmap, uint32_t n,
                                                         uint32_t early_n, const uint4* __restrict__ emsg,
                                                         uint4* __restrict__ m);
__global__ void __launch_bounds__(256) late_msgs_kernel(const uint32_t* __restrict__ rows,
                                                        const uint4* __restrict__ digs, uint32_t n,
                                                        uint8_t* __restrict__ m);

}  // namespace bcc
