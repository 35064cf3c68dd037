// wf_modelset.h — what modelset/wf_modelset.hip offers the rest of the library beyond the entries wf_handle.h declares: the
// validation of wf_set_model_sets on its own, and the device table of a handle that holds sets (calib/ writes into it).
#pragma once
#include <string>

#include "../wf_handle.h"

namespace wfi {

// What wf_set_model_sets asks of n sets: every field finite, ambient_ti > 0, and alpha, deflection alpha, ka TI + kb, deflection
// ka TI + kb, crespo_hernandez.constant > 0.  false: *why names the first set and field that fail.
bool modelset_validate(const wf_model_set* sets, int n, std::string* why);

// The device table of a handle that holds sets, [msets.size()] WfResolveConsts, brought up to date the way a step brings it:
// the model's constants first (wf_step: build_consts, which marks the table stale), then modelset_launch's check and upload.
// The step that follows finds nothing stale and leaves the table alone.  A function of its own, called by calib/ only:
// modelset_launch is as it was.  Whoever writes into the table owns the consequences: the host sets no longer describe it, and
// it is rebuilt from them when the sets, the model or the turbine count change.
int modelset_device_table(wf_handle* h, WfResolveConsts** tab);

}  // namespace wfi
