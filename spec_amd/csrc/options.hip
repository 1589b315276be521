// options.hip - the option surface of include/specmi.h: the table of every accepted name (default, stable / experimental) expanded
// from the one list in handle.h, the gate on experimental names, and the set / get / info entry points.
#include <cmath>
#include <cstdarg>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "handle.h"

using namespace specmi;

// ---- the option table: SPECMI_OPTIONS (handle.h) expanded to {name, default, stable}, indexed by enum Opt.  Names are strings only
// at the entry points below; the library itself reads its slots h->opt[] through opt() (handle.h).  Experimental names - tuning
// thresholds, debug pins, measured-slower opt-ins, the narrower-arithmetic secondary mode - are refused unless the process sets
// SPECMI_EXPERIMENTAL=1 or the handle's (stable) option "experimental" is 1; setting one to its default is always a no-op and
// allowed.  tests/test_abi.py checks the table against the header.
namespace {
struct OptSpec { const char* name; int def; bool stable; };
#define SPECMI_OPT(name, def, stable) {#name, def, stable},
const OptSpec kOptions[OPT_COUNT] = {SPECMI_OPTIONS(SPECMI_OPT)};
#undef SPECMI_OPT
int find_option(const char* name) {   // the Opt of a name, -1 = unknown
    for (int i = 0; i < OPT_COUNT; ++i)
        if (std::strcmp(kOptions[i].name, name) == 0) return i;
    return -1;
}
bool experimental_allowed(const specmi_handle* h) {
    const char* e = std::getenv("SPECMI_EXPERIMENTAL");
    if (e && e[0] && std::strcmp(e, "0") != 0) return true;
    return h->opt[OPT_experimental] != 0;
}
}  // namespace

specmi_handle::specmi_handle() {
    for (int i = 0; i < OPT_COUNT; ++i) opt[i] = kOptions[i].def;
}

extern "C" {

int specmi_set_option_i32(specmi_handle* h, const char* name, int value) {
    if (!h || !name) return fail(h, SPECMI_ERR_ARG, "null argument");
    const int o = find_option(name);
    if (o < 0) return fail(h, SPECMI_ERR_ARG, "unknown option '%s'", name);
    if (!kOptions[o].stable && value != kOptions[o].def && !experimental_allowed(h))
        return fail(h, SPECMI_ERR_STATE, "option '%s' is experimental (tuning / debug / measured-slower opt-in): set SPECMI_EXPERIMENTAL=1 "
                    "in the environment or option \"experimental\" = 1 on the handle first", name);
    h->opt[o] = value;
    return SPECMI_OK;
}

int specmi_set_option_f32(specmi_handle* h, const char* name, float value) {
    if (!h || !name) return fail(h, SPECMI_ERR_ARG, "null argument");
    if (std::strcmp(name, "focal_length") != 0) return fail(h, SPECMI_ERR_ARG, "unknown float option '%s'", name);
    h->focal_length = value;
    return SPECMI_OK;
}

int specmi_get_option_i32(specmi_handle* h, const char* name, int* value) {
    if (!h || !name || !value) return fail(h, SPECMI_ERR_ARG, "null argument");
    const int o = find_option(name);
    if (o < 0) return fail(h, SPECMI_ERR_ARG, "unknown option '%s'", name);
    *value = h->opt[o];
    return SPECMI_OK;
}

int specmi_option_info(int index, const char** name, int* default_value, int* is_stable) {
    if (index < 0 || index >= OPT_COUNT) return SPECMI_ERR_ARG;
    if (name) *name = kOptions[index].name;
    if (default_value) *default_value = kOptions[index].def;
    if (is_stable) *is_stable = kOptions[index].stable ? 1 : 0;
    return SPECMI_OK;
}

}  // extern "C"
