// What host code outside runtime.hip (note_objects.hip) needs of it: the thread's error text, the two failure macros and a view of the
// handle.  Private to csrc/: the public surface is include/ymt3.h.
#pragma once
#include "../../include/ymt3.h"
#include "common.h"
void ymt3_set_error(const char* fmt, ...);     // the text ymt3_last_error returns
#define FAIL(code, ...)              \
    do {                             \
        ymt3_set_error(__VA_ARGS__); \
        return (code);               \
    } while (0)
#define LAUNCH(expr)                                                             \
    do {                                                                         \
        int _rc = (expr);                                                        \
        if (_rc != 0) FAIL(YMT3_ERR_UNSUPPORTED, "%s rejected its shape (rc=%d)", #expr, _rc); \
    } while (0)
int handle_device(ymt3_handle h);              // struct ymt3_ctx itself stays in runtime.hip; h is not NULL
const ymt3_config& handle_config(ymt3_handle h);
