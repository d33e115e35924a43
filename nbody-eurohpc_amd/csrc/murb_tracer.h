// Host logic of the massless tracers (include/murbtracer.h has the definition): what an upload accepts, the option values, and
// how a set of tracers is cut into launches.  Pure host code that g++ compiles too, so that tests/test_tracer_host.py checks it
// through murbtracer_validate without a device.
//
// The planning is the field read-out's (murb_field_layout under "tracer_chunks" / "tracer_batch"): the chunk count is a function
// of the BODY count and of "tracer_chunks" alone, so a tracer's bits do not depend on how many tracers share its run.
#ifndef MURB_TRACER_H_
#define MURB_TRACER_H_

#include <cmath>
#include <cstring>

#include "murb_field.h"

// An upload's arguments: three position arrays, all or none of three velocity arrays, every value finite.
inline bool murb_tracer_upload_valid(unsigned long count, const float* const (&q)[3], const float* const (&v)[3])
{
    if (count == 0) return true;   // clears: the arrays are not read
    if (!q[0] || !q[1] || !q[2]) return false;
    const int nv = (v[0] != nullptr) + (v[1] != nullptr) + (v[2] != nullptr);
    if (nv != 0 && nv != 3) return false;
    for (const float* p : {q[0], q[1], q[2], v[0], v[1], v[2]})
        for (unsigned long i = 0; p && i < count; ++i)
            if (!std::isfinite(p[i])) return false;
    return true;
}

// "tracer_chunks" / "tracer_batch": the field options' values; "tracer_dt": 0 or 1.  false: no such key or a refused value.
inline bool murb_tracer_option_valid(const char* key, long value)
{
    if (!key) return false;
    if (!std::strcmp(key, "tracer_chunks")) return murb_field_options_valid(value, 0);
    if (!std::strcmp(key, "tracer_batch")) return murb_field_options_valid(0, value);
    if (!std::strcmp(key, "tracer_dt")) return value == 0 || value == 1;
    return false;
}

#endif
