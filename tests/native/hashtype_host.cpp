// Test-only: the product's job builder and host evaluation of sighash checks, without a device.
// build_sighash_checks (engine.cpp: add_sighash_job per check, as the deferring checker calls it)
// then host_sighash (host_verify.cpp: what host small rounds and the device-failure fallback run)
// over rows initialised to uint256 ONE.  Links the engine's host code of engine_host.so
// (tests/engine_stub.py), so the switch and the counts are that library's.
#include <cstdint>
#include <cstring>
#include <vector>

#include "bcc_amd.h"
#include "bcc_bench.h"
#include "host/engine.h"
#include "host/host_verify.h"

// Returns 0, or -1 when a check does not build.  msg32_out: 32 bytes per check; kinds: the job
// kinds the checks became (bcc_last_sighash_kinds); job_bytes (optional): the bytes a device round
// would upload for the jobs (padded preimages and aux messages, templates, code, raw txs, records).
extern "C" int hashtype_host_sighash(const bcc_sighash_check* checks, size_t n, uint8_t* msg32_out,
                                     bcc_sighash_kinds* kinds, size_t* job_bytes) {
    std::vector<bcc::host::SighashCheck> c(n);
    for (size_t i = 0; i < n; i++)
        c[i] = bcc::host::SighashCheck{checks[i].tx,          checks[i].tx_len,
                                       checks[i].script_code, checks[i].script_code_len,
                                       checks[i].n_in,        checks[i].hashtype,
                                       checks[i].amount,      checks[i].sigversion};
    bcc::SighashJobs jobs;
    bcc::TupleRows rows;
    if (bcc::host::build_sighash_checks(c.data(), n, jobs, rows) != n) return -1;
    if (rows.size() != n) return -1;
    for (size_t i = 0; i < n; i++) {
        memset(msg32_out + 32 * i, 0, 32);
        msg32_out[32 * i] = 1;
    }
    bcc::host::host_sighash(jobs, msg32_out);
    if (kinds) bcc_last_sighash_kinds(kinds);
    if (job_bytes)
        *job_bytes = jobs.aux.size() + jobs.pre.size() + jobs.tpl.size() + jobs.code.size() +
                     jobs.txraw.size() + sizeof(bcc::TplJob) * jobs.tjobs.size() +
                     sizeof(bcc::WtxRec) * jobs.wtx.size() + sizeof(bcc::WinJob) * jobs.wjobs.size() +
                     sizeof(bcc::LinJob) * jobs.ljobs.size() +
                     4 * (2 * jobs.aux_off.size() + 3 * jobs.pre_off.size()) +
                     sizeof(bcc::PatchRec) * jobs.patches.size();
    return 0;
}
