// wf_ext.h — the host layer every extension object (probe/, yawopt/, rose/, robust/, grad/, credit/, lookahead/, plan/, rollout/, retgrad/, policy/) stands on: the base
// struct with the parent handle, the error text and the event pool; a grow-only device buffer that frees itself; the
// evaluator — a further handle that follows the parent, configured through the public ABI of include/wfstep.h only; the
// checks an extension asks of its parent and of a farm list; the staging of a host caller's arrays (staging); event
// recording and the step / glue split of a timed run; kernel attributes; and the two drivers that enqueue a whole run on the
// parent's stream: run_rows — R evaluator rows for each of n items, in chunks: lay-out, one step, reduce (grad/, credit/,
// lookahead/, rollout/, retgrad/, rose/, robust/'s evaluation) — and run_search, the coordinate search over yaw of yawopt/ and robust/, with its
// configuration.  wf_ext.hip holds the non-template parts, wf_ext_kernels.h the device side.
// A new extension starts here: derive its object from ext_base, declare its buffers as dev_buf, and call these.
#pragma once
#include <cassert>
#include <cmath>
#include <functional>

#include "../wf_handle.h"
#include "wf_ext_kernels.h"

namespace wfi {

struct ext_base {
  wf_handle* h = nullptr;
  std::string err;
  // timing: events of the last run; per_chunk == 0: only its first and last, nothing to split
  int detail = 0;
  std::vector<hipEvent_t> ev_pool;
  size_t n_ev = 0, per_chunk = 0;
  bool timed = false;
  ~ext_base();
};

inline int ext_fail(ext_base* x, int code, const std::string& msg) {
  if (x) x->err = msg;
  return code;
}
#define WFX_HIP(x, call)                                                                             \
  do {                                                                                               \
    hipError_t e_ = (call);                                                                          \
    if (e_ != hipSuccess) return ext_fail(x, WF_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define WFX_EV(x, evh, call)                                                     \
  do {                                                                           \
    int rc_ = (call);                                                            \
    if (rc_ != WF_OK) return ext_fail(x, rc_, std::string("evaluator: ") + wf_last_error(evh)); \
  } while (0)
#define WFX_ON_DEVICE(x)                 \
  DeviceGuard guard_((x)->h->device);    \
  if (guard_.err != hipSuccess) return ext_fail(x, WF_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err))

// grow-only device buffer; freed with the object that holds it
template <class T>
struct dev_buf {
  T* p = nullptr;
  size_t cap = 0;
  dev_buf() = default;
  dev_buf(const dev_buf&) = delete;
  dev_buf& operator=(const dev_buf&) = delete;
  ~dev_buf() { hipFree(p); }
  operator T*() const { return p; }
};

// (the stream is drained before a buffer in use is released)
template <class T>
int reserve(ext_base* x, dev_buf<T>& buf, size_t n) {
  if (n <= buf.cap) return WF_OK;
  WFX_HIP(x, hipStreamSynchronize(x->h->stream));
  hipFree(buf.p);
  buf.p = nullptr; buf.cap = 0;
  WFX_HIP(x, hipMalloc(&buf.p, sizeof(T) * n));
  buf.cap = n;
  return WF_OK;
}

// an evaluator and what it was built from
struct evaluator {
  wf_handle* ev = nullptr;
  int E = 0, mode = -1;
  wf_model_params model{};
  std::vector<double> tws, tct, tcp, lx, ly;
  wf_kernel_choice choice{};
  int own_stage = -1;
  double guard = 0.0;
  hipStream_t stream = nullptr;
  evaluator() = default;
  evaluator(const evaluator&) = delete;
  evaluator& operator=(const evaluator&) = delete;
  ~evaluator() { if (ev) wf_destroy(ev); }
};
// A handle with the parent's model, layout, kernel choice and guard band on the parent's device and stream, E farms.
// Rebuilt (after draining the stream) when any of these differs from what it was built from; the resolve mode and the
// stream are just set.
int ensure_evaluator(ext_base* x, evaluator& s, int E, int mode);

// a farm list: the device copy and the host copy the upload reads from
struct farm_list {
  dev_buf<int> d;
  std::vector<int> host;
};

// what the checks of a wind process and of the ensemble's statistics (windgen/, ensemble/wf_ensemble_host.h) ask of a number
inline bool in_unit(double v) { return std::isfinite(v) && v >= 0.0 && v <= 1.0; }
inline bool non_negative(double v) { return std::isfinite(v) && v >= 0.0; }

// What a call asks of the parent: layout and batch, ONE layout, one turbine definition and, with `call`, a wind.  `what` is
// the extension's phrase with its verb ("yaw optimisation serves"), `call` the entry point's name (null: no wind needed).
int check_parent(ext_base* x, const char* what, const char* call);
int check_wind(ext_base* x, const char* call);
// ... and of its farm list; without one, n_farms becomes the parent's batch
int check_farms(ext_base* x, int* n_farms, const int* farms);
// the list on the device, fl.d reserved (a previous upload may still read the host copy: drain first)
int upload_farms(ext_base* x, farm_list& fl, const int* farms, int n_farms);

// the slots of the chunk that starts at entry `base` of the list (or of the batch), for an evaluator of C slots
inline WfSlots chunk_slots(const farm_list& fl, const int* farms, int base, int n_farms, int C) {
  return WfSlots{farms ? fl.d.p : nullptr, base, n_farms - base < C ? n_farms - base : C, C};
}

// A caller's arrays as the kernels see them.  A device caller's pointers pass through.  A host caller's arrays, of any
// element type, lie end to end (16-byte aligned) in `buf`, in the order they were named: in() for what the kernels read,
// out() for what they write; *d is the array's device pointer, null for a null array — a host caller's from begin() on.
struct staging {
  static constexpr int kMaxSegs = 15;  // the most arrays one call names (wf_polscen_run: two inputs, thirteen outputs)
  ext_base* x;
  dev_buf<char>& buf;
  bool host;
  struct seg { const void* src; void* user; size_t off, bytes; void* d; void (*set)(void* d, char* p); } segs[kMaxSegs];
  int n_segs = 0;
  size_t total = 0;
  staging(ext_base* x, dev_buf<char>& buf, int on_device) : x(x), buf(buf), host(!on_device) {}
  template <class T>
  void in(const T* src, size_t n, const T** d) {
    *d = src;
    if (host && src) add(seg{src, nullptr, total, sizeof(T) * n, d, [](void* d, char* p) { *(const T**)d = (const T*)p; }});
  }
  template <class T>
  void out(T* user, size_t n, T** d) {
    *d = user;
    if (host && user) add(seg{nullptr, user, total, sizeof(T) * n, d, [](void* d, char* p) { *(T**)d = (T*)p; }});
  }
  void add(const seg& s) { assert(n_segs < kMaxSegs); segs[n_segs++] = s; total += (s.bytes + 15) & ~(size_t)15; }
  int begin();  // reserves the buffer once, gives every array its place in it and enqueues the inputs' copies
  int end();    // after the run: a host caller's outputs come back, and the stream is drained
};

// the parent's fused env as the kernels see it: parameters by value, state by (read-only) pointer
inline WfEnvView env_view(const wf_handle* h) {
  WfEnvView e{};
  e.yaw = h->d_env_yaw; e.acc = h->d_env_acc; e.moves = h->d_env_moves;
  e.lo = h->env.yaw_lo; e.hi = h->env.yaw_hi; e.step = h->env.yaw_step;
  e.rate = h->env.actuator_rate; e.dt = h->env.dt; e.budget = h->env.budget; e.discrete = h->env.discrete;
  return e;
}

// an event on the parent's stream, from the pool
int record(ext_base* x);
// The last run's total, and with per_chunk != 0 its split: per chunk the events are e0 | glue e | step e | glue e | ... ,
// then the next chunk's e0 (an empty interval) — interval q of a chunk is a step when q is even and not 0.
int last_timing(ext_base* x, const char* not_run, float* total_ms, float* step_ms, float* glue_ms);
// numRegs, static LDS bytes and private-segment bytes of an extension's n kernels
int kernel_info(ext_base* x, int n, hipError_t (*attributes)(int, hipFuncAttributes*), int* info);

// ---- a row run: R evaluator rows for each of n items, in chunks (grad/, credit/, rose/, robust/'s evaluation) ----
// what a row-running object holds (grow-only): the evaluator's input and outputs, the rows' wind and the farm list
struct row_batch {
  dev_buf<float> d_yaw, d_pow, d_load;  // [E][N], [E][N], [E][N][4] (reserved for a policy with loads)
  dev_buf<double> d_wind;               // [2][E] speed, direction
  dev_buf<float> d_lws, d_lwd;          // [E][N] each: the step's local wind speed and direction (reserved for a policy with local_wind)
  farm_list farms;
};
// What differs between the row runs.  Every hook returns a WF_* code (and has set the error text).
struct row_policy {
  const char *what = "", *name = nullptr;  // check_parent's phrase and the entry point's name (null: the run needs no wind of the parent's)
  int rows = 1;             // evaluator rows an item takes
  std::string no_rows;      // ... <= 0 is refused with this, after the parent's checks
  const char* rows_msg = "";  // max_eval cannot hold one item's rows
  bool by_farm = true;      // an item is a farm: n_items and farms are check_farms'.  Else: no list, *n_items as it is after check
  int strict = 0, max_eval = 65536;
  bool loads = false;         // the step also fills d_load
  bool local_wind = false;    // the step also fills d_lws and d_lwd, its wind_speed / wind_dir outputs (policy/)
  bool split_always = false;  // four events per chunk on every run, not only under detail
  std::function<int()> check;  // the extension's own checks, after the parent's and the farm list's; may still set rows and *n_items
  std::function<int(int C, int E)> reserve;  // the extension's own buffers, for chunks of C items; names the caller's arrays to `st`
  // a chunk's kernels, before the step (yaw and wind of the E rows) and after it; sl.base is the chunk's first item
  std::function<int(const WfSlots& sl, int E)> layout, reduce;
  // A chunk may take several ROUNDS: rounds steps of the evaluator under the wind the lay-out wrote, with advance(sl, E, r),
  // r = 1 .. rounds - 1, between step r - 1 and step r: it reads the step's outputs and writes the next yaw block (plan/)
  int rounds = 1;
  std::function<int(const WfSlots& sl, int E, int round)> advance;
  std::function<int()> finish;  // what follows the last chunk, if anything (the rose's copy of its sums)
};
// The whole run on the parent's stream.  Chunks of C = max_eval / rows items (at most all *n_items), E = C rows evaluator
// farms.  Per chunk: layout, then wf_set_wind_counts from b.d_wind and one wf_step from b.d_yaw into b.d_pow (and b.d_load),
// then — under a policy of several rounds — advance and one more wf_step per further round; the driver sets the wind once per
// chunk, and an advance hook that writes another wind into b.d_wind calls wf_set_wind_counts itself before it returns (policy/);
// then reduce.  With local_wind every step also writes b.d_lws / b.d_lwd.  The caller's arrays go through `st`: begun after
// reserve, ended last.  Events: the run's first and last, or
// split per chunk e0 | lay-out e | wind + step e | advance e | step e | ... | reduce e (last_timing's per_chunk layout with
// 2 rounds + 2: 4 for one round).
int run_rows(ext_base* x, row_batch& b, evaluator& es, row_policy& k, staging& st, int* n_items, const int* farms);

// ---- the coordinate search over yaw (include/wfyawopt.h; include/wfrobust.h: "with farm power replaced by E") ----
struct search_config {
  double lo = -25.0, hi = 25.0;
  int P = 2, K[WF_SEARCH_MAX_PASSES] = {5, 4, 0, 0};
  int strict = 0, max_eval = 65536;
};
// The validating setter.  rows_per_candidate: evaluator rows a candidate row takes (1; the robust search's members, 1 before
// any are set); rows_msg: the refusal when max_eval_farms cannot hold one farm's rows.
int set_search_config(ext_base* x, search_config& c, double lo, double hi, int n_passes, const int* K, int strict, int max_eval_farms,
                      int rows_per_candidate, const char* rows_msg);
// the passes: K_max, and the grids h_0 = (hi - lo) / (K_0 - 1), h_p = 2 h_{p-1} / (K_p + 1)
int k_max(int P, const int* K);
void pass_grids(double lo, double hi, int P, const int* K, WfGrid* grid);

// what a searching object holds: the configuration, a row run's buffers (the wind is the extension's to fill) and the
// device buffers (grow-only) every search needs besides
struct yaw_search : row_batch {
  search_config cfg;
  dev_buf<float> d_best;    // [C][N] best yaw so far
  dev_buf<int> d_order;     // [C][N]
  dev_buf<char> d_stage;    // staging for host callers: yaw0, yaw_opt, power_opt, power_init
};

// What differs between the searches.  Every hook returns a WF_* code (and has set the error text).
struct search_policy {
  const char *what, *name;  // check_parent's phrase and the entry point's name
  int rows_per_candidate;   // evaluator rows a candidate row takes: 1, or the robust search's members
  std::string no_rows;      // ... <= 0 is refused with this, after the parent's checks
  const char* rows_msg;     // max_eval_farms cannot hold one farm's rows
  std::function<int(int E)> reserve;  // the extension's own buffers for E evaluator farms; nothing is enqueued yet
  std::function<int(const WfSlots&, int R, int E)> begin_chunk;  // the evaluator's wind for this chunk, then the order kernel
  std::function<int(const WfAdvanceArgs&, int v)> visit;  // launch v: what turns the powers of visit v - 1 into the yaw of visit v
};
// The whole search on the parent's stream, the arguments those of wf_yawopt_run.  Chunks of C slots of R = K_max + 1 candidate
// rows, E = C R rows_per_candidate evaluator farms.  Per chunk: begin_chunk, then launches v = 0 .. V (V = P N visits), each
// followed — for v < V — by one wf_step on the evaluator from s.d_yaw into s.d_pow.  Events: the run's first and last, or with
// detail per chunk e0 | glue e | step e | glue e | ... | glue e (2 V + 2; last_timing's per_chunk layout).
int run_search(ext_base* x, yaw_search& s, evaluator& es, const search_policy& k, const float* yaw0, int n_farms, const int* farms,
               float* yaw_opt, float* power_opt, float* power_init, int on_device);

template <class T>
int ext_create(wf_handle* h, T** out) {
  if (!h || !out) return WF_E_INVALID;
  *out = nullptr;
  T* x = new (std::nothrow) T();
  if (!x) return fail(h, WF_E_NOMEM, "out of host memory");
  x->h = h;
  *out = x;
  return WF_OK;
}

// (the object's members go in reverse order of declaration: evaluators, declared last, before the buffers; the events after)
template <class T>
int ext_destroy(T* x) {
  if (!x) return WF_OK;
  DeviceGuard guard(x->h->device);
  hipStreamSynchronize(x->h->stream);
  delete x;
  return WF_OK;
}

}  // namespace wfi
