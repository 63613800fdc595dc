// The last-error message of libbrever_sdr.so (include/brever_sdr.h): the library's own thread-local string, written
// through brv::fail (../status.h) by its translation units and read through brv_sdr_last_error().
#include "../../../include/brever_sdr.h"
#include "../status.h"

namespace {
thread_local std::string g_err;
}

int brv::fail(int code, const char* msg) { g_err = msg ? msg : ""; return code; }

extern "C" {

int brv_sdr_version(void) { return 100; }
const char* brv_sdr_last_error(void) { return g_err.c_str(); }

}
