// The last-error message of libbrever_resample.so (include/brever_resample.h): the library's own thread-local
// string, written through brv::fail (../status.h) by its translation units and read through brv_rs_last_error().
#include "../../../include/brever_resample.h"
#include "../status.h"

namespace {
thread_local std::string g_err;
}

int brv::fail(int code, const char* msg) { g_err = msg ? msg : ""; return code; }

extern "C" {

int brv_rs_version(void) { return 100; }
const char* brv_rs_last_error(void) { return g_err.c_str(); }

}
