// rf_trace_wide_list.hpp -- the kTraceWide instantiations this build ships, as one list: X(any-hit, counting build, nearest-first, record layout, dense leaf phase).
// rf_trace.hip expands it into the table of kernel addresses (traceWideKernel), the host-only launch policy into traceWideInstantiated (rf_launch_policy.cpp): the
// policy resolves a launch to an instantiation without linking device code.
// The layouts the renderer picks by itself (+ the oct records, an option), each closest-hit one and the any-hit variants it pairs them with; with the dense leaf
// phase only where a default launch can reach it (rf_launch_policy.cpp: planBounce / resolveTraversal)
#pragma once

#if defined(RF_EXP_LEGACY_LAYOUTS)
#define RF_TRACE_WIDE_LEGACY_INSTANTIATIONS(X) X(false, false, false, 1, false) X(false, false, false, 2, false) X(true, false, true, 1, false) X(true, false, true, 2, false)
#else
#define RF_TRACE_WIDE_LEGACY_INSTANTIATIONS(X)
#endif

#define RF_TRACE_WIDE_INSTANTIATIONS(X) \
    X(false, true, false, 0, false) X(true, true, true, 0, false) X(true, true, false, 0, false) \
    X(false, false, false, 0, false) X(false, false, false, 3, false) X(false, false, false, 4, false) X(false, false, false, 5, false) X(false, false, false, 6, false) \
    X(false, false, false, 3, true) X(false, false, false, 4, true) X(false, false, false, 5, true) \
    X(true, false, true, 0, false) X(true, false, false, 0, false) \
    X(true, false, true, 3, false) X(true, false, false, 3, false) X(true, false, true, 4, false) X(true, false, false, 4, false) X(true, false, true, 5, false) X(true, false, false, 5, false) \
    X(true, false, true, 3, true) X(true, false, false, 4, true) X(true, false, false, 5, true) \
    RF_TRACE_WIDE_LEGACY_INSTANTIATIONS(X)
