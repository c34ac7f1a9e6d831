// xsd_err.h -- the library's one error formatter: every translation unit reports a failure through it.
#pragma once

namespace xsd {
// formats the thread-local message that xsd_last_error() returns and hands `code` back: `return failf(XSD_ERR_ARG, "...", ...)`.
// Defined in xsd_engine.hip; internal to the library (hidden: no dynamic symbol)
__attribute__((visibility("hidden"), format(printf, 2, 3))) int failf(int code, const char* fmt, ...);
}
