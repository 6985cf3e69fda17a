// What a smtts_handle points to, shared by the units that define extern "C" entries (capi.hip, deliver.hip).
#pragma once
#include <string>

#include "engine.hpp"

struct smtts_engine {
    Engine e;
    explicit smtts_engine(int dev) : e(dev) {}
};
extern thread_local std::string g_create_err;   // capi.hip: what smtts_last_error(NULL) returns

#define E (h->e)
// every entry point that takes a handle rejects NULL with an error code (message via smtts_last_error(NULL))
#define NULLCHK if (!h) { g_create_err = std::string(__func__) + ": null handle"; return 1; }
#define NULLCHK0 if (!h) { g_create_err = std::string(__func__) + ": null handle"; return 0; }
#define ST(s) static_cast<hipStream_t>(s)
