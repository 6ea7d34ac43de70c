// Shared host helpers of libscgpu.so: the thread-local error message behind
// scg_last_error() and HIP launch checks.
#pragma once

namespace scg {

// Record a printf-style message for scg_last_error() and return `code`.
int fail(int code, const char* fmt, ...);

// SCG_ERR_HIP (with the HIP error string) if the last launch failed, else SCG_OK.
int check_launch(const char* what);

// A stream as the step servers' host lifecycle sees it (scg_server_host.h): idle when all
// its work has completed, busy while some is queued or running, or a HIP error (*text: its
// string); and the blocking wait for it, true on success.
enum StreamState { kStreamIdle, kStreamBusy, kStreamError };
StreamState stream_state(void* stream, const char** text);
bool stream_wait(void* stream);

}  // namespace scg
