// bcc_verify_inputs_batch (inputs.cpp) keeps a second caller thread per calling thread.
#pragma once

namespace bcc {
namespace host {

// Releases the state the calling thread's second caller keeps (its team, device batches and job
// buffers) and joins it (bcc_release_thread_state).
void inputs_release_thread_state();

}  // namespace host
}  // namespace bcc
