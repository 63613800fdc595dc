// The library's last-error message (include/brever_hip.h): one thread-local string, written through
// brv::fail (status.h) by every translation unit and read through brv_last_error().
#include "../../include/brever_hip.h"
#include "status.h"

namespace {
thread_local std::string g_err;
}

int brv::fail(int code, const char* msg) { g_err = msg ? msg : ""; return code; }

extern "C" {

int brv_version(void) { return 100; }
const char* brv_last_error(void) { return g_err.c_str(); }

}
