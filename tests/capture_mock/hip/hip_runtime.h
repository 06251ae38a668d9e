// Scripted mock of the seven HIP runtime calls lemo_amd/csrc/engine_host.hpp makes, for tests/capture_helper_main.cpp: every call is
// recorded in mock::log, and a call fails with mock::fail[call] when that is non-zero.  Graphs and execs are heap blocks, so the
// address sanitizer reports a graph destroyed twice or never.
#pragma once
#include <cstddef>
#include <vector>

typedef int hipError_t;
enum { hipSuccess = 0 };
typedef struct mockStream* hipStream_t;
struct mockGraph { int alive; };
struct mockExec { int alive; };
typedef mockGraph* hipGraph_t;
typedef mockExec* hipGraphExec_t;
enum hipStreamCaptureMode { hipStreamCaptureModeGlobal, hipStreamCaptureModeThreadLocal, hipStreamCaptureModeRelaxed };

namespace mock {
enum Call { BEGIN, END, INSTANTIATE, UPLOAD, GRAPH_DESTROY, EXEC_DESTROY, LAUNCH, NCALL };
struct State {
  int fail[NCALL] = {};
  std::vector<int> log;
  hipStreamCaptureMode mode = hipStreamCaptureModeGlobal;
  bool capturing = false;
  bool end_hands_graph_on_failure = false;   // hipStreamEndCapture may or may not hand a graph back when it fails
  int count(Call c) const { int n = 0; for (int x : log) n += x == c; return n; }
};
inline State& st() { static State s; return s; }
inline int note(Call c) { st().log.push_back(c); return st().fail[c]; }
}  // namespace mock

inline hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode m) {
  if (int e = mock::note(mock::BEGIN)) return e;
  mock::st().mode = m; mock::st().capturing = true;
  return hipSuccess;
}
inline hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t* g) {
  const int e = mock::note(mock::END);
  mock::st().capturing = false;
  *g = (!e || mock::st().end_hands_graph_on_failure) ? new mockGraph{1} : nullptr;
  return e;
}
inline hipError_t hipGraphInstantiate(hipGraphExec_t* x, hipGraph_t g, void*, void*, size_t) {
  const int e = mock::note(mock::INSTANTIATE);
  if (!g || !g->alive) return 1;
  *x = e ? reinterpret_cast<hipGraphExec_t>(0x1) : new mockExec{1};      // a failed instantiate leaves garbage behind
  return e;
}
inline hipError_t hipGraphUpload(hipGraphExec_t x, hipStream_t) {
  const int e = mock::note(mock::UPLOAD);
  return (x && x->alive) ? e : 1;
}
inline hipError_t hipGraphDestroy(hipGraph_t g) {
  mock::note(mock::GRAPH_DESTROY);
  delete g;
  return hipSuccess;
}
inline hipError_t hipGraphExecDestroy(hipGraphExec_t x) {
  mock::note(mock::EXEC_DESTROY);
  delete x;
  return hipSuccess;
}
inline hipError_t hipGraphLaunch(hipGraphExec_t x, hipStream_t) {
  const int e = mock::note(mock::LAUNCH);
  return (x && x->alive && !mock::st().capturing) ? e : 1;
}
