// build_knobs.h -- every compile-time knob of the library, fenced.
//
// The sources carry shape parameters of the sweeps quoted in profiles/ (AMT_LIN_G, AMT_TILE_WAVES ...) and host-side call tracing
// (AMT_TRACE_CALLS).  The release library is built with NONE of them (amatsukaze_amd/build.py FLAGS / EXTRA_FLAGS,
// tests/test_abi_and_host.py); a stray -DAMT_LIN_G=3 in a packager's CXXFLAGS must not produce a library that is silently
// different.  Any of them without AMT_INSTRUMENTED_BUILD -- which only build.py's build_variant() sets, and which names the product
// libamt_gpu_<variant>.so -- is a compile error.  The evaluation kernels' ablations (AMT_*_NO_*: wrong results by design), phase timers
// (AMT_*_TIMING) and AMT_EXPERIMENT are retired: a compile error in every build.  Included first by every source of the library.
#pragma once

#if defined(AMT_LIN_NO_EVAL) || defined(AMT_LIN_NO_FIXUP) || defined(AMT_LIN_NO_FLUSH) || defined(AMT_LIN_NO_CONVERT) || defined(AMT_LIN_RAW_SAMEFRAME) || \
    defined(AMT_PAIR_NO_SUM) || defined(AMT_PAIR_NO_EVAL) || defined(AMT_PAIR_NO_CONVERT) || defined(AMT_PAIR_NO_FLUSH) || defined(AMT_PAIR_NO_GATHER) || \
    defined(AMT_PAIR_NO_RAW) || defined(AMT_PAIR_RAW_SAMEFRAME) || defined(AMT_LIN_TIMING) || defined(AMT_PAIR_TIMING) || defined(AMT_FUSED_TIMING) || \
    defined(AMT_EXPERIMENT)
#error "a retired switch (AMT_*_NO_* / *_RAW_SAMEFRAME / AMT_*_TIMING / AMT_EXPERIMENT) is defined: the ablations and phase timers were removed from the evaluation kernels, so this define would silently time the release kernel, also in a build_variant; the last commit that has them is f05270e (Cadence renderer: edge-directed, motion-adaptive bob for 60i frames)"
#endif
#if !defined(AMT_INSTRUMENTED_BUILD)
#if defined(AMT_TRACE_CALLS)
#error "AMT_TRACE_CALLS (host-side call tracing) is defined outside an instrumented build (amatsukaze_amd/build.py build_variant)"
#endif
#if defined(AMT_LIN_G) || defined(AMT_LIN_G16) || defined(AMT_LIN_OCC) || defined(AMT_LIN_OCC16) || defined(AMT_LIN_WAVES) || defined(AMT_LIN_WGS_MIN16) || \
    defined(AMT_TILE_WAVES) || defined(AMT_TILE_G) || defined(AMT_PAIR_OCC) || defined(AMT_LISTED_FADE_CHUNK) || \
    defined(AMT_STATS_ROWS) || defined(AMT_STATS_ROWS8) || defined(AMT_STATS_RUN) || defined(AMT_STATS_NT) || defined(AMT_STATS_WAVES) || \
    defined(AMT_DELOGO_ROWS) || defined(AMT_DELOGO_FRAMES)
#error "a shape / tuning macro of the kernels is defined on the command line: the release library is built with the defaults in the sources (instrumented variants: amatsukaze_amd/build.py build_variant)"
#endif
#endif
