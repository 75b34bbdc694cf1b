// error.cpp -- the thread-local error text behind vbm25_last_error, and the library's version.  No HIP: plain g++.

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "vbm25_internal.h"

namespace vbm25 {

static thread_local char g_error[ERROR_TEXT_BYTES] = "";

int set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return code;
}

void error_text_read(char *out) { std::memcpy(out, g_error, sizeof g_error); }
void error_text_write(const char *in) { std::memcpy(g_error, in, sizeof g_error); }

}  // namespace vbm25

extern "C" {

const char *vbm25_last_error(void) { return vbm25::g_error; }
const char *vbm25_version(void) { return "vbm25-mi355x 0.1 (gfx950)"; }

}  // extern "C"
