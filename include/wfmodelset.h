/* wfmodelset.h — wake-model parameter sets per farm: an extension of libwfstep.so (include/wfstep.h).
 *
 * A handle solves every farm of its batch under one wf_model_params.  Wind, layout, turbine definition and yaw may differ
 * per farm; with this extension the flow and wake-model constants may too: ambient turbulence intensity, shear, veer, the
 * Gaussian expansion set, the deflection set and Crespo-Hernandez — the eighteen fields of wf_model_set.  Uses: domain
 * randomisation (training across perturbed wake parameters), robustness evaluation (one wind, one action, an ensemble of
 * wake models in one launch), calibration (S candidate sets scored against measured powers in one step).
 *
 * COST, stated plainly: while sets are held EVERY farm is solved by the float64 kernels on EVERY step (csrc/wf_resolve_ms.hip,
 * csrc/wf_resolve4_ms.hip — the float32 kernels, their pair tables and their risk flags know one model).  That is the path of
 * wf_set_risk_resolve(2) and of wf_set_turbine_types: wf_get_risk_resolve reports 2, wf_set_risk_resolve(0) is refused, and
 * the mode set before is in force again once the sets are cleared.  The feature is off until wf_set_model_sets is called.
 *
 * What a set may change is exactly the fields below.  Everything else stays the handle's model: air_density, the rotor, the
 * hub height, the turbine scalars and table, the GCH internals and the three solver switches.  Geometry (the sort, ties, the
 * 15 D reach, the 2 D gate) depends on D alone and is untouched.  Each set's constants are built by the code that builds the
 * handle's own (csrc/wf_model.hip: fill_resolve_consts): a set equal to the model gives the same bytes, hence the same bits.
 *
 * Composition: turbine definitions (wf_set_turbine_types), several layouts (set_of is per farm as layout_of is), the fused
 * env step (the float64 kernels write the reward).  wf_set_model and wf_set_layout with another turbine count are honoured:
 * the table is rebuilt from the stored sets at the next step, the fields outside a set following the new model.
 * wf_set_batch with another batch invalidates set_of: the next step fails and says to set the sets again.
 *
 * OUT OF SCOPE: the extensions that evaluate the single model (everything behind check_parent of csrc/ext/wf_ext.hip: rose,
 * robust, yawopt, grad, credit, lookahead, plan, rollout, retgrad, scenario, ...) and the flow probe (include/wfprobe.h, which
 * carries one set of constants) refuse a handle that holds sets with WF_E_UNSUPPORTED, by name.
 * wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFMODELSET_H
#define WFMODELSET_H

#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wf_model_set {
  double ambient_ti, shear, veer, alpha, beta, ka, kb, ad, bd, dm,
         ch_initial, ch_constant, ch_ai, ch_downstream,
         defl_alpha, defl_beta, defl_ka, defl_kb;
} wf_model_set;

/* n_sets sets and the set of each farm; set_of NULL: n_sets == env_batch, farm b takes set b.  1 <= n_sets <= env_batch;
 * n_sets == 0 clears the sets.  WF_E_INVALID, by name: a call before wf_set_batch, a set_of entry outside 0..n_sets-1, a
 * non-finite field, ambient_ti <= 0, and what wf_set_model refuses of these fields (alpha, deflection alpha, ka TI + kb,
 * deflection ka TI + kb, crespo_hernandez.constant not > 0). */
int wf_set_model_sets(wf_handle* h, int n_sets, const wf_model_set* sets, const int* set_of);
/* the sets in force: *n_sets (0: none); sets [n_sets] and set_of [env_batch] may be NULL */
int wf_get_model_sets(wf_handle* h, int* n_sets, wf_model_set* sets, int* set_of);
/* the handle's model as a set: the starting point of a perturbation */
int wf_model_set_from_model(wf_handle* h, wf_model_set* out);
/* which float64 kernel served the last step with sets: *waves_per_farm = 4 (four-wave kernel), 1 (one-wave kernel), 0 (none yet) */
int wf_model_sets_last_kernel(wf_handle* h, int* waves_per_farm);

#ifdef __cplusplus
}
#endif
#endif
