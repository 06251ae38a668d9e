// Host-side plumbing every engine shares (lemo_hip.hip, lemo_prox.hip, ae_engine.hip, ae_train_engine.hip, prior_train_engine.hip):
// the return-on-error macro, stream-capture of a launch sequence into a hipGraphExec, its replay, and the release of graph handles.
// Needs nothing but the HIP runtime API and the C ABI's error codes, so tests/capture_helper_main.cpp compiles it against a scripted mock.
#pragma once
#include <hip/hip_runtime.h>
#include "lemo_hip.h"

#define S(x) ((hipStream_t)(x))
#define CHK(e) do { int _e = (e); if (_e) return _e; } while (0)

namespace lemo {

// Capture what body() enqueues on s (ThreadLocal mode: other threads' runtime calls do not invalidate it) into *out.
// A capture that was begun is always ended, and its graph is destroyed once on every path.  Returns the first failure of body(),
// hipStreamEndCapture, hipGraphInstantiate, in that order; on any failure *out is null (the engines replay every non-null handle).
// upload: hand the graph to the device now, so that the first replay does not pay for it (lemo_fit_prepare).
template <class F>
static int capture_graph(hipGraphExec_t* out, hipStream_t s, bool upload, F&& body) {
  *out = nullptr;
  CHK((int)hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  int rc = body();
  hipGraph_t g = nullptr;
  const int ec = (int)hipStreamEndCapture(s, &g);
  if (!rc) rc = ec;
  if (!rc) rc = (int)hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  if (g) (void)hipGraphDestroy(g);
  if (rc) { *out = nullptr; return rc; }
  if (upload) (void)hipGraphUpload(*out, s);
  return 0;
}

// n runs of body() on s.  use_graph: captured once into *exec (kept by the caller across calls; a failed capture leaves it null, so
// the next call captures again) and launched n times.  Returns the first failure; n <= 0 does nothing.
template <class F>
static int replay_or_run(hipGraphExec_t* exec, bool use_graph, int n, hipStream_t s, F&& body) {
  if (use_graph && !*exec && n > 0) CHK(capture_graph(exec, s, false, body));
  for (int i = 0; i < n; ++i) CHK(use_graph ? (int)hipGraphLaunch(*exec, s) : body());
  return 0;
}

static inline void destroy_graphs(hipGraphExec_t* a, int n) {
  for (int i = 0; i < n; ++i)
    if (a[i]) { (void)hipGraphExecDestroy(a[i]); a[i] = nullptr; }
}

}  // namespace lemo
