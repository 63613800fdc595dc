// The last-error message of libbrever_flacenc.so (include/brever_flacenc.h): the library's own thread-local string,
// written through brv::fail (../status.h) by its translation units and read through brv_flacenc_last_error().
#include "../../../include/brever_flacenc.h"
#include "../status.h"

namespace {
thread_local std::string g_err;
}

int brv::fail(int code, const char* msg) { g_err = msg ? msg : ""; return code; }

extern "C" {

int brv_flacenc_version(void) { return 100; }
const char* brv_flacenc_last_error(void) { return g_err.c_str(); }

}
