// Stand-alone check of lemo::capture_graph / lemo::replay_or_run / lemo::destroy_graphs (lemo_amd/csrc/engine_host.hpp) against the scripted runtime in
// tests/capture_mock: the error paths no GPU test can reach.  Built and run by tests/test_capture_helper.py with
// -fsanitize=address,undefined, so a graph destroyed twice or leaked fails the run as well.  Prints one line per case; exit 0 = all hold.
#include "engine_host.hpp"

#include <cstdio>
#include <cstring>

using namespace mock;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

struct Run { int rc, body_runs; hipGraphExec_t out; };

// one capture_graph call on a fresh script: `fail_call` (or none: NCALL) fails with `code`; the body returns body_rc
static Run run(Call fail_call, int code, int body_rc, bool upload, bool graph_on_end_failure = false) {
  st() = State();
  if (fail_call != NCALL) st().fail[fail_call] = code;
  st().end_hands_graph_on_failure = graph_on_end_failure;
  Run r{0, 0, reinterpret_cast<hipGraphExec_t>(0x2)};     // a stale handle: failures must not leave it
  r.rc = lemo::capture_graph(&r.out, nullptr, upload, [&] {
    ++r.body_runs;
    EXPECT(st().capturing && st().mode == hipStreamCaptureModeThreadLocal);
    return body_rc;
  });
  EXPECT(!st().capturing);
  EXPECT(st().count(GRAPH_DESTROY) <= 1);
  return r;
}

// lemo::replay_or_run: what the training engines' step and epoch loops are made of
static void replay_cases() {
  int bodies = 0, body_rc = 0;
  auto body = [&] { ++bodies; return body_rc; };
  auto captures = [] { return st().count(BEGIN) + st().count(END) + st().count(INSTANTIATE); };
  hipGraphExec_t exec = nullptr;

  std::printf("replay, eager: n bodies, no capture call\n");
  st() = State();
  EXPECT(lemo::replay_or_run(&exec, false, 3, nullptr, body) == 0);
  EXPECT(bodies == 3 && exec == nullptr && st().log.empty());

  std::printf("replay, eager: the first body failure ends the loop\n");
  bodies = 0; body_rc = LEMO_ERR_SHAPE;
  EXPECT(lemo::replay_or_run(&exec, false, 3, nullptr, body) == LEMO_ERR_SHAPE && bodies == 1 && st().log.empty());

  std::printf("replay, graph, n = 0: no capture\n");
  bodies = 0; body_rc = 0;
  EXPECT(lemo::replay_or_run(&exec, true, 0, nullptr, body) == 0);
  EXPECT(bodies == 0 && exec == nullptr && st().log.empty());

  std::printf("replay, graph: a body failure inside the capture is returned, nothing is launched, the next call captures again\n");
  body_rc = LEMO_ERR_ARG;
  EXPECT(lemo::replay_or_run(&exec, true, 2, nullptr, body) == LEMO_ERR_ARG);
  EXPECT(bodies == 1 && exec == nullptr && !st().capturing);
  EXPECT(st().count(BEGIN) == 1 && st().count(END) == 1 && st().count(INSTANTIATE) == 0 && st().count(LAUNCH) == 0);

  std::printf("replay, graph, first call: one begin / end / instantiate, n launches\n");
  st() = State();
  bodies = 0; body_rc = 0;
  EXPECT(lemo::replay_or_run(&exec, true, 3, nullptr, body) == 0);
  EXPECT(bodies == 1 && exec != nullptr && captures() == 3 && st().count(UPLOAD) == 0 && st().count(LAUNCH) == 3);
  const int order[7] = {BEGIN, END, INSTANTIATE, GRAPH_DESTROY, LAUNCH, LAUNCH, LAUNCH};
  EXPECT((int)st().log.size() == 7 && std::memcmp(st().log.data(), order, sizeof(order)) == 0);

  std::printf("replay, graph, second call: no capture, n launches\n");
  st() = State();
  const hipGraphExec_t kept = exec;
  EXPECT(lemo::replay_or_run(&exec, true, 2, nullptr, body) == 0);
  EXPECT(bodies == 1 && exec == kept && captures() == 0 && st().count(LAUNCH) == 2 && st().log.size() == 2);

  std::printf("replay, graph: a launch failure is returned at once, the graph is kept\n");
  st() = State();
  st().fail[LAUNCH] = 17;
  EXPECT(lemo::replay_or_run(&exec, true, 3, nullptr, body) == 17);
  EXPECT(bodies == 1 && exec == kept && st().count(LAUNCH) == 1 && st().log.size() == 1);
  lemo::destroy_graphs(&exec, 1);
}

int main() {
  std::printf("begin fails: the body is not run\n");
  {
    Run r = run(BEGIN, 7, 0, true);
    EXPECT(r.rc == 7 && r.body_runs == 0 && r.out == nullptr);
    EXPECT(st().count(END) == 0 && st().count(INSTANTIATE) == 0 && st().count(GRAPH_DESTROY) == 0);
  }
  std::printf("body fails: its code, capture ended, graph destroyed once\n");
  {
    Run r = run(NCALL, 0, LEMO_ERR_SHAPE, true);
    EXPECT(r.rc == LEMO_ERR_SHAPE && r.body_runs == 1 && r.out == nullptr);
    EXPECT(st().count(END) == 1 && st().count(GRAPH_DESTROY) == 1 && st().count(INSTANTIATE) == 0 && st().count(UPLOAD) == 0);
  }
  std::printf("body and end fail: the body's code wins\n");
  {
    Run r = run(END, 9, LEMO_ERR_ARG, true);
    EXPECT(r.rc == LEMO_ERR_ARG && r.out == nullptr && st().count(END) == 1 && st().count(INSTANTIATE) == 0);
  }
  std::printf("end fails, with and without a graph handed back\n");
  for (int handed = 0; handed < 2; ++handed) {
    Run r = run(END, 9, 0, true, handed != 0);
    EXPECT(r.rc == 9 && r.body_runs == 1 && r.out == nullptr);
    EXPECT(st().count(INSTANTIATE) == 0 && st().count(UPLOAD) == 0 && st().count(GRAPH_DESTROY) == handed);
  }
  std::printf("instantiate fails\n");
  {
    Run r = run(INSTANTIATE, 11, 0, true);
    EXPECT(r.rc == 11 && r.out == nullptr);
    EXPECT(st().count(GRAPH_DESTROY) == 1 && st().count(UPLOAD) == 0);
  }
  for (int upload = 0; upload < 2; ++upload) {
    std::printf("success %s upload\n", upload ? "with" : "without");
    Run r = run(NCALL, 0, 0, upload != 0);
    EXPECT(r.rc == 0 && r.body_runs == 1 && r.out != nullptr && r.out != reinterpret_cast<hipGraphExec_t>(0x2));
    EXPECT(st().count(GRAPH_DESTROY) == 1 && st().count(UPLOAD) == upload);
    const int order[5] = {BEGIN, END, INSTANTIATE, GRAPH_DESTROY, UPLOAD};
    EXPECT((int)st().log.size() == 4 + upload && std::memcmp(st().log.data(), order, sizeof(int) * (4 + upload)) == 0);
    hipGraphExec_t a[3] = {nullptr, r.out, nullptr};
    lemo::destroy_graphs(a, 3);                           // skips the null entries, clears the one it destroyed
    EXPECT(st().count(EXEC_DESTROY) == 1 && a[1] == nullptr);
    lemo::destroy_graphs(a, 3);
    EXPECT(st().count(EXEC_DESTROY) == 1);
  }
  std::printf("upload fails: the graph is still usable\n");
  {
    Run r = run(UPLOAD, 13, 0, true);
    EXPECT(r.rc == 0 && r.out != nullptr);
    lemo::destroy_graphs(&r.out, 1);
  }
  replay_cases();
  std::printf(failures ? "%d checks failed\n" : "all capture_graph checks hold\n", failures);
  return failures ? 1 : 0;
}
