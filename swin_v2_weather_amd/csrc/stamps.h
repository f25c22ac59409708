// In-kernel phase timing of the diagnostic builds (tools/build_stamped.sh, tools/probe_*stamps*.py): a wave accumulates s_memtime deltas
// per phase in st_acc[] and the kernel leaves them where its probe reads them.  A file defines SWV2_STAMPS under its own -D switch
// before it includes this header; without it every macro is empty and the production build carries nothing.
//   STAMP_DECL(n)      the counters (n phases)              STAMP_START()        first reading
//   STAMP(k)           phase k ends here                    STAMP_DEP(k, dep)    ... ordered behind the value `dep` that ends the phase
//   STAMP_DRAINED(k)   ... behind the wave's outstanding LDS / scalar operations (they are charged to phase k, not to the next)
//   STAMP_WAITV()      wait for the wave's vector-memory operations (so the next stamp charges them to its phase)
#pragma once
#ifdef SWV2_STAMPS
#define STAMP_CLOCK(t, pre, ...) asm volatile(pre "s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : __VA_ARGS__ : "memory")
#define STAMP_AT(k, pre, ...) do { unsigned long long t_; STAMP_CLOCK(t_, pre, __VA_ARGS__); st_acc[k] += t_ - st_prev; st_prev = t_; } while (0)
#define STAMP_DECL(n) unsigned long long st_prev = 0, st_acc[n] = {};
#define STAMP_START() do { STAMP_CLOCK(st_prev, ""); } while (0)
#define STAMP(k) STAMP_AT(k, "")
#define STAMP_DEP(k, dep) STAMP_AT(k, "", "v"(dep))
#define STAMP_DRAINED(k) STAMP_AT(k, "s_waitcnt lgkmcnt(0)\n\t")
#define STAMP_WAITV() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define STAMP_DECL(n)
#define STAMP_START() do {} while (0)
#define STAMP(k) do {} while (0)
#define STAMP_DEP(k, dep) do {} while (0)
#define STAMP_DRAINED(k) do {} while (0)
#define STAMP_WAITV() do {} while (0)
#endif
