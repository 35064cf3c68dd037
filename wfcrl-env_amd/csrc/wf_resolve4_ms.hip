// wf_resolve4_ms.hip — part 2 of wf_resolve.hip for wake-model parameter sets per farm (see wf_resolve_ms.hip, wf_resolve4.hip).
#define RES_MT 1
#define RES_MS 1
#define RES_PART 2
#include "wf_resolve.hip"
