// wf_resolve_ms.hip — the float64 farm solve of wf_resolve.hip compiled for wake-model parameter sets per farm
// (include/wfmodelset.h: wf_set_model_sets): kernels wf_resolve_ms_kernel / wf_resolve4_ms_kernel, entry wfk_launch_resolve_ms.
// Built on the several-definitions build (RES_MT: a handle without turbine definitions runs with one definition made from its
// model).  See the RES_MS block at the top of wf_resolve.hip for what differs.
#define RES_MT 1
#define RES_MS 1
#include "wf_resolve.hip"
