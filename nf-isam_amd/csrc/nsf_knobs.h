// nsf_knobs.h -- every environment switch of libnfisam_hip.so: one table, one accessor per switch.
// Plain host C++17 (no HIP include), and the only file of csrc/ that calls getenv.  INTEGRATION.md §6 has one row per line of
// the table below and tests/test_knobs_cpu.py holds the two together.
// WHEN a switch is read is part of its contract:
//   CALL  at every call of its accessor.  A test may flip it inside its own process.
//   ONCE  once per PROCESS, at the first call of its accessor (one static local of a non-template inline function for the
//         whole library).  Later changes of the environment are not seen: a test sets it in a child process's environment.
// KIND, i.e. the parse:
//   OFF    bool, default true;  false when the value's first character is '0'
//   ON     bool, default false; true when the value's first character is '1'
//   SET    bool: the variable exists, whatever it holds
//   CHAR   int: the value's first character (0 for an empty value), -1 when unset; the launcher compares it
//   WORD   bool name(word): the whole value equals `word`
//   INT    int: atoi of the value, the default when unset; name_set(): the variable exists.  The LAUNCHER validates
//          (NFISAM_BIG_W and NFISAM_TILES_PER_BLOCK have one rule per kernel family)
//   CLAMP  int: atoi of the value (the default when unset) clamped to lo .. hi
//   REAL   double: atof of the value, the default when unset
#pragma once
#include <limits.h>
#include <stdlib.h>
#include <string.h>

//     accessor         variable                   when  kind   lo hi       default  meaning
#define NSF_KNOBS(X) \
    X(train,           "NFISAM_TRAIN",            CALL, WORD,  0, 0,       0,    "wide | split: force the 64-particle or the two-lanes-per-particle training kernels (default: by launch)") \
    X(dim_major,       "NFISAM_DIM_MAJOR",        CALL, OFF,   0, 0,       1,    "0: one-layer training launches through the tile-major kernels instead of nsf_train1_kernel") \
    X(big_w,           "NFISAM_BIG_W",            CALL, INT,   1, 8,       4,    "waves per block: dim-major kernel 1, 2, 4 or 8; tile-major wide kernel 1 .. 8; anything else is 4") \
    X(tiles_per_block, "NFISAM_TILES_PER_BLOCK",  CALL, INT,   1, 8,       0,    "64-particle tiles per gradient copy: dim-major 1, 2, 4 or 8; tile-major 1 .. 8; anything else: by launch size") \
    X(half,            "NFISAM_HALF",             CALL, CHAR,  0, 0,       -1,   "two lanes per particle on the dim-major kernel: 0 never, 2 also groups of nine to sixteen blocks") \
    X(fused_adam,      "NFISAM_FUSED_ADAM",       CALL, OFF,   0, 0,       1,    "0: a separate nsf_adam_kernel launch per iteration (and no chunk-persistent form)") \
    X(pair_image,      "NFISAM_PAIR_IMAGE",       CALL, OFF,   0, 0,       1,    "0: nsf_train3_kernel stages its panels from the parameters in every launch") \
    X(pair,            "NFISAM_PAIR",             CALL, CHAR,  0, 0,       -1,   "multi-layer / dL/dx launches: 0 never nsf_train3_kernel, 1 for every width it holds (default: from D = 6)") \
    X(pair_stash,      "NFISAM_PAIR_STASH",       CALL, OFF,   0, 0,       1,    "0: nsf_train3_kernel recomputes the lower layers in its backward pass instead of parking them") \
    X(dim_pairing,     "NFISAM_DIM_PAIRING",      CALL, OFF,   0, 0,       1,    "0: nsf_train2_kernel's wave w takes dim w") \
    X(lean,            "NFISAM_LEAN",             CALL, OFF,   0, 0,       1,    "0: never the two-waves-per-SIMD build of the dim-major kernels") \
    X(walk,            "NFISAM_WALK",             CALL, WORD,  0, 0,       0,    "plain: the one-lane-per-sample posterior walk") \
    X(chains,          "NFISAM_CHAINS",           CALL, INT,   1, 8,       0,    "launches per iteration of a one-layer plan, clamped to 1 .. 8 and to the octets of groups (unset: by launch size)") \
    X(span,            "NFISAM_SPAN",             CALL, ON,    0, 0,       0,    "1: a single-clique plan's whole run as one window-spanning launch (read per plan)") \
    X(span_debug,      "NFISAM_SPAN_DEBUG",       CALL, SET,   0, 0,       0,    "print whether a plan got the window-spanning graph") \
    X(probe_debug,     "NFISAM_PROBE_DEBUG",      CALL, SET,   0, 0,       0,    "print what the co-residency probe saw") \
    X(run_ahead,       "NFISAM_RUN_AHEAD",        CALL, OFF,   0, 0,       1,    "0: a plan run waits for a chunk's outcome before it enqueues the next (read per run)") \
    X(persist,         "NFISAM_PERSIST",          ONCE, OFF,   0, 0,       1,    "0: one-layer plans always launch one kernel per iteration") \
    X(persist_probe,   "NFISAM_PERSIST_PROBE",    ONCE, OFF,   0, 0,       1,    "0: plan creation does not launch the co-residency probe") \
    X(fused_close,     "NFISAM_FUSED_CLOSE",      ONCE, OFF,   0, 0,       1,    "0: a chunk-persistent chunk is closed by two kernels instead of one") \
    X(wait_seconds,    "NFISAM_WAIT_SECONDS",     ONCE, REAL,  0, 0,       60.0, "seconds a plan run waits for a chunk before it gives up on a wedged stream") \
    X(plan_stream,     "NFISAM_PLAN_STREAM",      ONCE, WORD,  0, 0,       0,    "private: replay the chunks' graphs on the plan's own stream behind an event hand-over") \
    X(persist_direct,  "NFISAM_PERSIST_DIRECT",   ONCE, OFF,   0, 0,       1,    "0: a chunk-persistent chunk is replayed as its captured graph instead of two launches") \
    X(slab_max_tiles,  "NFISAM_SLAB_MAX_TILES",   ONCE, CLAMP, 0, INT_MAX, 128,  "most per-tile gradient copies before one copy + float atomics; the workspace size and the launches share it") \
    X(lone_lean,       "NFISAM_LONE_LEAN",        ONCE, OFF,   0, 0,       1,    "0: lone launches keep the three-wave build of the chunk-persistent kernel") \
    X(helpers,         "NFISAM_HELPERS",          ONCE, OFF,   0, 0,       1,    "0: four waves per block, no helper waves") \
    X(persist_split,   "NFISAM_PERSIST_SPLIT",    ONCE, CHAR,  0, 0,       -1,   "set: 1 divides the Adam update among a group's blocks, anything else does not (unset: above 256 blocks)") \
    X(persist_spins,   "NFISAM_PERSIST_SPINS",    ONCE, CLAMP, 1, 26,      15,   "log2 of the looks a block waits at its group barrier; 1 .. 26: the window-spanning kernel shifts 1u by this + 5") \
    X(persist_drop,    "NFISAM_PERSIST_DROP",     ONCE, ON,    0, 0,       0,    "1 (test): one block of one group leaves at once; the run must end with NFISAM_ERR_STALL") \
    X(persist_scatter, "NFISAM_PERSIST_SCATTER",  ONCE, ON,    0, 0,       0,    "1 (test): transpose the grid so that a group's blocks sit on different XCDs")

namespace knob {
// ---- the parses: pure functions of the variable's value (nullptr: unset) -------------------------------------------------------
inline bool flag_off(const char* e) { return !(e != nullptr && e[0] == '0'); }
inline bool flag_on(const char* e) { return e != nullptr && e[0] == '1'; }
inline bool is_set(const char* e) { return e != nullptr; }
inline int first_char(const char* e) { return e != nullptr ? (int)(unsigned char)e[0] : -1; }
inline bool word_is(const char* e, const char* w) { return e != nullptr && strcmp(e, w) == 0; }
inline int int_or(const char* e, int dflt) { return e != nullptr ? atoi(e) : dflt; }
inline int int_clamped(const char* e, int lo, int hi, int dflt) { const int v = int_or(e, dflt); return v < lo ? lo : (v > hi ? hi : v); }
inline double real_or(const char* e, double dflt) { return e != nullptr ? atof(e) : dflt; }
// what the launchers validate an INT with: v when it is one of / lies in, else the fallback
inline int int_in_set(int v, int a, int b, int c, int d, int fallback) { return (v == a || v == b || v == c || v == d) ? v : fallback; }
inline int int_in_range(int v, int lo, int hi, int fallback) { return (v >= lo && v <= hi) ? v : fallback; }
// a ONCE switch keeps its own copy of the value: the environment may change under a pointer that getenv returned
inline const char* kept(const char* e) { return e != nullptr ? strdup(e) : nullptr; }
#define NSF_KNOB_VALUE_CALL(var) const char* const e = getenv(var);
#define NSF_KNOB_VALUE_ONCE(var) static const char* const e = kept(getenv(var));
#define NSF_KNOB_OFF(fn, var, when, lo, hi, dflt)   inline bool fn() { NSF_KNOB_VALUE_##when(var) return flag_off(e); }
#define NSF_KNOB_ON(fn, var, when, lo, hi, dflt)    inline bool fn() { NSF_KNOB_VALUE_##when(var) return flag_on(e); }
#define NSF_KNOB_SET(fn, var, when, lo, hi, dflt)   inline bool fn() { NSF_KNOB_VALUE_##when(var) return is_set(e); }
#define NSF_KNOB_CHAR(fn, var, when, lo, hi, dflt)  inline int fn() { NSF_KNOB_VALUE_##when(var) return first_char(e); }
#define NSF_KNOB_WORD(fn, var, when, lo, hi, dflt)  inline bool fn(const char* w) { NSF_KNOB_VALUE_##when(var) return word_is(e, w); }
#define NSF_KNOB_INT(fn, var, when, lo, hi, dflt)   inline int fn() { NSF_KNOB_VALUE_##when(var) return int_or(e, dflt); } \
                                                    inline bool fn##_set() { NSF_KNOB_VALUE_##when(var) return is_set(e); }
#define NSF_KNOB_CLAMP(fn, var, when, lo, hi, dflt) inline int fn() { NSF_KNOB_VALUE_##when(var) return int_clamped(e, lo, hi, dflt); }
#define NSF_KNOB_REAL(fn, var, when, lo, hi, dflt)  inline double fn() { NSF_KNOB_VALUE_##when(var) return real_or(e, dflt); }
#define NSF_KNOB_ACCESSOR(fn, var, when, kind, lo, hi, dflt, meaning) NSF_KNOB_##kind(fn, var, when, lo, hi, dflt)
NSF_KNOBS(NSF_KNOB_ACCESSOR)
}   // namespace knob
