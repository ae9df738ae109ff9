// The seam between bcc_taproot_spend_batch's host pass (host/taproot_spend.cpp) and its fused
// device round (taproot_commit.hip): one round's script-path commitments and signature checks,
// and the hook through which the host code reaches the device.  csrc/host is also built into the
// CPU tests' device-less engine, which defines only the older device seams; there no hook is set
// and the round runs as commitment lane code on the host + gpu_taproot_verify_parts.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "bcc_amd.h"
#include "pipeline.h"

namespace bcc {

// A queued tapscript signature check's TapLeaf hash: the round's commitment lane that computes it
// and the byte offset of the check's slot in its part's ext blob (TapJob.ext_off plus 32 bytes for
// each of sha_annex and sha_single_output the job carries).
struct LeafCopy {
    uint32_t lane;
    uint32_t ext_byte;
};

// One part of a round, built by one host thread over a contiguous item range.
struct SpendPart {
    TaprootJobs jobs;                          // key-path and queued tapscript checks, in item order
    std::vector<LeafCopy> copies;              // lane relative to this part's commits
    std::vector<bcc_taproot_commit> commits;   // the part's script-path items (valid control size)
};

struct SpendRound {
    SpendPart* const* parts;
    size_t P;
};

// begin: stages, uploads and queues the whole round on `slot`'s stream (TAPROOT_SLOTS contexts per
// thread and device, as gpu_taproot_begin) and returns; the parts may be rebuilt afterwards.
// end: waits once and writes the commitment verdicts (one byte per commitment, parts in order) and
// the signature verdicts (one byte per row, parts in order).  Each begin is matched by an end.
struct SpendDeviceHook {
    int (*begin)(int device, int slot, const SpendRound& round);
    int (*end)(int device, int slot, uint8_t* commit_verdict, uint8_t* sig_verdict);
};
// Set by the translation unit that owns the kernels when the library loads; null without one.
extern const SpendDeviceHook* g_spend_device_hook;

}  // namespace bcc
