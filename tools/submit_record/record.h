// record.h -- what the recording fake (fake_hip.cpp) offers the programs that drive it (driver.cpp, split_ops_record.cpp, cursor_raycast_record.cpp, listed_ops_record.cpp, light_rays_record.cpp and the two check programs).
#pragma once
#include <string>

void rec(const char *fmt, ...) __attribute__((format(printf, 1, 2)));  // one line of the record
std::string rec_ptr(const void *p);   // "null", "A<allocation ordinal>+<offset>" or "host"
void fake_reset();                    // a scenario starts: ordinals from zero (every allocation of the last one has been freed)
void fake_fail(const char *fn, int nth);  // the nth call of the runtime function or Split-operation launcher `fn` from now on (0 = the next) fails, once
int fake_calls(const char *fn);       // calls of `fn` since fake_reset
void fake_bail(bool on);              // the trace stub reports a wave that gave up (DevCounters::bailed)
struct aic_ctx;
extern int (*fake_light_job_finish)(aic_ctx *);  // when set, the stub of light_job_finish calls it (light_rays_record.cpp: a pending update is finished first)
