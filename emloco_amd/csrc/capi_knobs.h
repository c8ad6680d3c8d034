// capi_knobs.h -- internal, host only: the environment knobs that select a kernel variant inside the library, read once (the first time
// a launch consults them) and parsed strictly.  The launchers and emloco_kernel_variants (predictor_capi.hip) read the SAME functions,
// so what the export reports is what is launched.  One instance per knob for the whole library (inline functions: their statics are
// shared by every translation unit).
//   EMLOCO_ATTN_BWD_PIECES   2 | 3     pieces per operand of the split-mode attention backward            (unset: 2)
//   EMLOCO_ATTN16_OLD        0 | 1     round 4's attention kernels for the bf16-memory and split modes    (unset: 0)
//   EMLOCO_GEMM_WIDE_STORES  0 | 1     16-byte epilogue stores of whole output lines                      (unset: 1)
//   EMLOCO_GEMM_BK           16 | 32   a forced stage depth of the GEMM family                            (unset: 0 = by launch shape)
// Any other value (an empty string included) is refused: the first launch that consults the knob returns EMLOCO_E_ARG through
// capi_fail with a text that names the variable and its value, and so does every later one.
#pragma once
#include <stdlib.h>
#include <string>
#include "capi_error.h"

namespace emloco {

struct Knob {
    int value;             // the parsed value; -1 when the variable holds something else
    std::string refusal;   // empty, or the text of the refusal
};

// `unset` when the variable is not in the environment, a or b when it spells exactly that decimal number
inline Knob knob_parse(const char *name, int unset, int a, int b) {
    const char *e = getenv(name);
    if (!e) return {unset, {}};
    const std::string s(e);
    if (s == std::to_string(a)) return {a, {}};
    if (s == std::to_string(b)) return {b, {}};
    return {-1, std::string(name) + "=" + s + ": not one of the accepted values " + std::to_string(a) + " and " + std::to_string(b)};
}

inline const Knob &knob_attn_bwd_pieces() { static const Knob k = knob_parse("EMLOCO_ATTN_BWD_PIECES", 2, 2, 3); return k; }
inline const Knob &knob_attn16_old() { static const Knob k = knob_parse("EMLOCO_ATTN16_OLD", 0, 0, 1); return k; }
inline const Knob &knob_gemm_wide_stores() { static const Knob k = knob_parse("EMLOCO_GEMM_WIDE_STORES", 1, 0, 1); return k; }
inline const Knob &knob_gemm_bk() { static const Knob k = knob_parse("EMLOCO_GEMM_BK", 0, 16, 32); return k; }

// the refusal of a launch (or of the report) that consulted a knob with a value outside its list: "who: VARIABLE=value: ..."
inline int knob_fail(const char *who, const Knob &k) { return capi_fail(EMLOCO_E_ARG, who, k.refusal.c_str()); }

}  // namespace emloco

// ends the entry point it stands in when the knob holds a refused value
#define EMLOCO_KNOBCHK(knob)                                                             \
    do {                                                                                 \
        const emloco::Knob &k_ = (knob);                                                 \
        if (k_.value < 0) return emloco::knob_fail(__func__, k_);                        \
    } while (0)
