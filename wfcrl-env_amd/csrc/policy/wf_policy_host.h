// wf_policy_host.h — the host-side checks of a network that the policy extension (wf_policy_abi.hip) and the extension that
// runs the same network over a wind ensemble (polscen/wf_polscen_abi.hip) share, so that neither restates the other's:
// what wf_policy_set_network validates and lays out, and what a run checks of the network against its parent.  Defined in
// wf_policy_abi.hip.
#pragma once
#include <vector>

#include "../ext/wf_ext.h"
#include "wf_policy.h"

namespace wfi {

// wf_policy_set_network's arguments, validated (include/wfpolicy.h names the refusals) -> the network's lay-out and the
// normalisation [2][D] (shift, scale); `net` and `norm` are written only when WF_OK is returned
int policy_network(ext_base* x, int kind, int n_layers, const int* widths, int activation, int final, int use_freewind, double out_scale,
                   const double* shift, const double* scale, WfPolicyNet* net, std::vector<double>* norm);

// what a run checks of a network against its parent h: the input width of its kind, the output width of the env's action
// encoding, the parameter count P; sets net.discrete
int policy_network_fits(ext_base* x, const wf_handle* h, WfPolicyNet& net, int P);

}  // namespace wfi
