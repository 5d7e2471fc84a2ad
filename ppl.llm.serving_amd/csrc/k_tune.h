// The tuning switches of the launch heuristics (host only, no HIP header: the launch plan of linear_plan.cc reads them too).
#pragma once
#include <stdlib.h>

namespace pplhip {

// Tuning switches of the launch heuristics (tile shapes, ring depths, split-K counts ...): the PRODUCT reads none of them -- the values the
// measurements of profiles/ settled on are compiled in.  A tuning build (make TUNING=1: -DPPLHIP_TUNING_BUILD) reads them from the
// environment, which is what the sweep scripts under profiles/probes/ use.  (Switches the product does read -- collectives, schedules,
// the A/B switches of recent changes -- are listed in INTEGRATION.md with their defaults.)
inline int tune_int(const char* name, int dflt) {
#ifdef PPLHIP_TUNING_BUILD
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
#else
    (void)name;
    return dflt;
#endif
}
inline bool tune_set(const char* name) {
#ifdef PPLHIP_TUNING_BUILD
    return getenv(name) != nullptr;
#else
    (void)name;
    return false;
#endif
}

}  // namespace pplhip
