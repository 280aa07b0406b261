/*
 * engine_tuning.h — the engine's tuning switches as a value.  tuning_from_env() reads every OHEVC_* variable the engine knows,
 * once, when the engine is created (engine.hip: engine_create); nothing else in the engine looks at the environment, so two
 * engines of one process may differ and a variable set later is simply not seen.  Pure host code: no HIP runtime call, no engine —
 * tests/intra_plan_check.cpp runs it on the CPU.  The table of the switches is DESIGN.md §4d.
 */
#ifndef OHEVC_ENGINE_TUNING_H
#define OHEVC_ENGINE_TUNING_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

enum { OH_INTRA_AUTO = 0, OH_INTRA_DAG, OH_INTRA_DIRECT };

struct OhTuning {
    int      intra_mode = OH_INTRA_AUTO; /* OHEVC_INTRA_MODE=dag / direct: one form of the intra pass for every picture; anything else: by content */
    uint32_t intra_waves = 0;            /* OHEVC_INTRA_WAVES: waves per CTU of the staged form, 2, 4 or 8 (any other value: 8); 0, unset: by content */
    uint32_t intra_phases = 2;           /* OHEVC_INTRA_PHASES: groups of waves the sub-levels go round; must suit the waves (intra_plan.h), else 2 */
    int      intra_res_lds = -1;         /* OHEVC_INTRA_RES_LDS: 0 / 1 the CTUs' residual spans fetched per block / staged in LDS; -1, unset: by launch size */
    uint32_t spin_limit = 1u << 22;      /* OHEVC_SPIN_LIMIT: polls (with s_sleep between them, ~1 s in all) before a waiting workgroup gives up */
    int      copy_threads = 2;           /* OHEVC_COPY_THREADS: helper threads of the hand-over, 0..8; 0: the submitter does everything alone */
    int      fetch_threads = 3;          /* OHEVC_FETCH_THREADS: helper threads of the output fetch, 0..15 */
    bool     stamps = false;             /* OHEVC_STAMPS: room for the in-kernel stamp records of a -DOH_STAMPS build */
    bool     fetch_timing = false;       /* OHEVC_FETCH_TIMING: where the time of the fetches went, printed when the engine is destroyed */
};

static inline OhTuning tuning_from_env()
{
    OhTuning t;
    if (const char *v = getenv("OHEVC_INTRA_MODE"))
        t.intra_mode = !strcmp(v, "dag") ? OH_INTRA_DAG : !strcmp(v, "direct") ? OH_INTRA_DIRECT : OH_INTRA_AUTO;
    if (const char *v = getenv("OHEVC_INTRA_WAVES")) {
        t.intra_waves = (uint32_t)atoi(v);
        if (t.intra_waves != 2 && t.intra_waves != 4 && t.intra_waves != 8) t.intra_waves = 8;
    }
    if (const char *v = getenv("OHEVC_INTRA_PHASES"))
        t.intra_phases = (uint32_t)atoi(v);                  /* judged against the launch's waves: intra_plan.h */
    if (const char *v = getenv("OHEVC_INTRA_RES_LDS"))
        t.intra_res_lds = atoi(v) != 0;
    if (const char *v = getenv("OHEVC_SPIN_LIMIT"))          /* tests: make a waiting workgroup give up at once */
        t.spin_limit = (uint32_t)std::max(1l, atol(v));
    if (const char *v = getenv("OHEVC_COPY_THREADS"))
        t.copy_threads = std::max(0, std::min(atoi(v), 8));
    if (const char *v = getenv("OHEVC_FETCH_THREADS"))
        t.fetch_threads = std::max(0, std::min(atoi(v), 15));
    t.stamps = getenv("OHEVC_STAMPS") != nullptr;
    t.fetch_timing = getenv("OHEVC_FETCH_TIMING") != nullptr;
    return t;
}

#endif
