// trk_loop_kind.h -- "the running channels of a closed-loop engine are of one kind", as a pure host function.  Compiles without
// HIP (tests/loop_kind_selftest.cpp prints the decision of any argument tuple; tests/test_loop_kind.py holds a table worked out by
// hand against it).
#ifndef TRK_LOOP_KIND_H
#define TRK_LOOP_KIND_H

enum LoopFamily
{
    LOOP_VEML = 0,     // gc_trk_loop_start: the persistent kernel, or the mixed one
    LOOP_GLONASS = 1,  // gc_trk_loop_start_glonass: its own kernel and state
    LOOP_MODE = 2      // a request only: a change of the engine's mode (gc_trk_loop_set_mixed), for no channel
};

// what one launch's kernel is instantiated for: of the engine's running channels, or of the channel a start asks for
struct LoopKind
{
    int family;
    int n_taps, pilot, high_dyn;  // LOOP_VEML only
};

enum LoopKindVerdict
{
    LOOP_ADMIT = 0,
    LOOP_REFUSE_RUNNING,        // the mode changes only while no channel runs
    LOOP_REFUSE_GLONASS_RUNS,   // a veml start while a GLONASS channel runs
    LOOP_REFUSE_VEML_RUNS,      // a GLONASS start while a veml channel runs
    LOOP_REFUSE_MIXED_GLONASS,  // a mixed engine has no GLONASS slots
    LOOP_REFUSE_TAPS,
    LOOP_REFUSE_PILOT,
    LOOP_REFUSE_HIGH_DYN
};

// cur: the kind the engine was last started with -- it binds only while channels run.  others_started: a channel other than the
// requested one runs; any_started: any channel does.  A slot restarted while it alone runs may change taps, pilot and high_dyn
// (nothing else is left of the old kind); it may not change family, because the two families keep their state in different buffers
// and the slot's stop is what hands it over.  In a mixed engine taps and pilot are per channel, high_dyn is the launch's.
static inline LoopKindVerdict loop_kind_admit(const LoopKind& cur, bool mixed, bool others_started, bool any_started, const LoopKind& req)
{
    if (req.family == LOOP_MODE) return any_started ? LOOP_REFUSE_RUNNING : LOOP_ADMIT;
    if (req.family == LOOP_GLONASS)
        {
            if (mixed) return LOOP_REFUSE_MIXED_GLONASS;
            return any_started && cur.family != LOOP_GLONASS ? LOOP_REFUSE_VEML_RUNS : LOOP_ADMIT;
        }
    if (any_started && cur.family == LOOP_GLONASS) return LOOP_REFUSE_GLONASS_RUNS;
    if (!others_started) return LOOP_ADMIT;
    if (!mixed && cur.n_taps != req.n_taps) return LOOP_REFUSE_TAPS;
    if (!mixed && cur.pilot != req.pilot) return LOOP_REFUSE_PILOT;
    if (cur.high_dyn != req.high_dyn) return LOOP_REFUSE_HIGH_DYN;
    return LOOP_ADMIT;
}

#endif
