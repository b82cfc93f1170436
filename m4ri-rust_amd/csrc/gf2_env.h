// gf2_env.h -- environment knobs and word arithmetic shared by the planner and the executing units (no HIP)
#pragma once
#include <cstdlib>
static inline int words_of(int bits) { return (bits + 63) >> 6; }
static inline int env_int(const char *name, int dflt) {
  const char *e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}
// Fitted model constants and A/B switches: read from the environment in development builds only (tools/libm4ri_hip_dev.so,
// built with -DGF2K_DEV_VARIANTS; the A/B scripts under tools/ load it through AB_LIB).  The shipped library uses the default:
// INTEGRATION.md section 6 lists which variables it still reads.
#ifdef GF2K_DEV_VARIANTS
#define dev_env_int(name, dflt) env_int(name, dflt)
#else
#define dev_env_int(name, dflt) (dflt)
#endif
