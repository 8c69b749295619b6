// The guard around a C entry that works on a resident set, for the set classes of the host layer (NavFactorSet, PreintegrationSetT,
// MarginalizationPriorSet): the entry is in this build (missing: the name of one that is not, else null), a set is resident (ctx), the call
// returned ICG_OK.  Otherwise *err says which, in the entry's own words once it was called.
#pragma once
#include <string>

#include "../../include/icgvins_hip.h"

namespace icg {
template <class Call> inline bool residentCall(const char *missing, icg_ctx *ctx, const std::string &no_set, std::string *err, Call call) {
    const bool ok = !missing && ctx && call() == ICG_OK;
    if (!ok && err) *err = missing ? std::string(missing) + " is not in this build" : ctx ? icg_last_error(ctx) : no_set;
    return ok;
}
} // namespace icg
