// libmpn.so runtime glue: error string shared by every entry point.
#include "mpn_common.h"
#include <stdarg.h>
#include <stdlib.h>

namespace mpn {
static thread_local std::string g_err;
void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}
const char *get_error() { return g_err.c_str(); }
thread_local Arena *tl_arena = nullptr;
thread_local bool tl_oom = false;
std::atomic<long long> g_arena_bytes{0};
long long arena_test_budget() {
    static const long long b = []() { const char *e = getenv("MPN_TEST_ARENA_BUDGET"); return e ? atoll(e) : 0LL; }();
    return b;
}
}  // namespace mpn

extern "C" const char *mpn_last_error(void) { return mpn::get_error(); }
