// hipemu -- a tiny HOST emulation of the HIP device model.   TEST INFRASTRUCTURE ONLY.
//
// Purpose: this container has no GPU and every GPU call costs budgeted minutes, so the CPU test
// suite compiles the *unmodified* kernel sources of lemo_amd/csrc with a host compiler against
// this header (it shadows <hip/hip_runtime.h> on the include path) and checks index arithmetic,
// MFMA operand / accumulator lane maps and host orchestration against the oracle before any GPU
// time is spent.  It is NOT a product path: lemo_amd never loads the emulated library, the
// product loader only opens liblemo_hip.so built by hipcc for gfx950.
//
// Model: every thread of a block is a fiber on ONE OS thread, scheduled round-robin; __syncthreads / cross-lane
// ops / MFMA are generation barriers that yield.  The blocks of a launch are spread over up to HIPEMU_THREADS OS
// threads (default min(8, cores)); `__shared__`, threadIdx & co and the scheduler state are thread_local.  Results do
// not depend on the thread count: atomicAdd (the kernels never use its return value) is LOGGED per block and applied
// after the launch in block order = exactly the order of the one-thread emulator.
// Wavefront = 64 lanes.  MFMA f32 lane maps follow /opt/skills/guides/cdna_hip_programming.md §3:
//   32x32x2 : A[i=l&31][k=l>>5]  B[k=l>>5][j=l&31]  D: col=l&31, row=(r&3)+8*(r>>2)+4*(l>>5)
//   16x16x4 : A[i=l&15][k=l>>4]  B[k=l>>4][j=l&15]  D: col=l&15, row=4*(l>>4)+r
// and numerics are a k-ordered fmaf chain (bit-exact per the guide).
#pragma once
#include <link.h>
#include <sys/mman.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

#define HIPEMU 1
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __noinline__ __attribute__((noinline))
#define __shared__ static thread_local
#define LEMO_PIN(x) ((void)0)
#define __launch_bounds__(...)
#define __constant__ static

struct dim3 {
  unsigned x, y, z;
  constexpr dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct alignas(16) float4 { float x, y, z, w; };
struct int2 { int x, y; };
struct alignas(16) int4 { int x, y, z, w; };
struct uint2 { unsigned x, y; };
struct alignas(16) uint4 { unsigned x, y, z, w; };
static inline float2 make_float2(float x, float y) { return {x, y}; }
static inline float3 make_float3(float x, float y, float z) { return {x, y, z}; }
static inline float4 make_float4(float x, float y, float z, float w) { return {x, y, z, w}; }
static inline int2 make_int2(int x, int y) { return {x, y}; }
static inline int4 make_int4(int x, int y, int z, int w) { return {x, y, z, w}; }
static inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { return {x, y, z, w}; }
static inline uint2 make_uint2(unsigned x, unsigned y) { return {x, y}; }

typedef void* hipStream_t;
typedef void* hipGraph_t;
typedef void* hipGraphExec_t;
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorInvalidConfiguration = 9, hipErrorNotSupported = 801 };
enum hipMemcpyKind { hipMemcpyHostToHost, hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice, hipMemcpyDefault };
enum hipStreamCaptureMode { hipStreamCaptureModeGlobal, hipStreamCaptureModeThreadLocal, hipStreamCaptureModeRelaxed };
static inline const char* hipGetErrorString(hipError_t) { return "hipemu"; }
static inline hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return hipSuccess; }
static inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
static inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
static inline hipError_t hipDeviceSynchronize() { return hipSuccess; }
static inline hipError_t hipMalloc(void** p, size_t n) { *p = aligned_alloc(256, (n + 255) / 256 * 256); return *p ? hipSuccess : 2; }
static inline hipError_t hipFree(void* p) { free(p); return hipSuccess; }
enum hipFuncAttribute { hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
enum hipDeviceAttribute_t { hipDeviceAttributeMaxSharedMemoryPerBlock = 74 };
static inline hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) { return hipErrorNotSupported; }
static inline hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t*) { return hipErrorNotSupported; }
static inline hipError_t hipGraphInstantiate(hipGraphExec_t*, hipGraph_t, void*, void*, size_t) { return hipErrorNotSupported; }
static inline hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { return hipErrorNotSupported; }
static inline hipError_t hipGraphUpload(hipGraphExec_t, hipStream_t) { return hipErrorNotSupported; }
static inline hipError_t hipGraphDestroy(hipGraph_t) { return hipSuccess; }
static inline hipError_t hipGraphExecDestroy(hipGraphExec_t) { return hipSuccess; }
typedef void* hipEvent_t;
static inline hipError_t hipEventCreate(hipEvent_t* e) { *e = nullptr; return hipSuccess; }
static inline hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
static inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
enum { hipStreamNonBlocking = 1, hipEventDisableTiming = 2 };
static inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = nullptr; return hipSuccess; }      // null = "no second stream"
static inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { *s = nullptr; return hipSuccess; }
static inline hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 0; *hi = 0; return hipSuccess; }
static inline hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
static inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = nullptr; return hipSuccess; }
static inline hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
static inline hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
static inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }

namespace hipemu {

constexpr int WAVE = 64;
constexpr size_t STACK = 256 * 1024;

struct Group { int count = 0, arrived = 0; unsigned gen = 0; };
struct WaveBuf {
  Group g;
  float a[WAVE], b[WAVE];
  float c[WAVE][16];
  unsigned long long u[WAVE];
  float a8[WAVE][8], b8[WAVE][8];
};
// Minimal x86-64 fiber switch (callee-saved registers + stack pointer).  glibc's swapcontext makes a
// sigprocmask syscall per switch, which dominated the emulation time (2 switches per lane per MFMA).
struct Ctx { void* sp = nullptr; };
extern "C" void hipemu_switch(Ctx* from, Ctx* to);
asm(R"(
.text
.weak hipemu_switch
.type hipemu_switch,@function
hipemu_switch:
    pushq %rbp
    pushq %rbx
    pushq %r12
    pushq %r13
    pushq %r14
    pushq %r15
    movq %rsp, (%rdi)
    movq (%rsi), %rsp
    popq %r15
    popq %r14
    popq %r13
    popq %r12
    popq %rbx
    popq %rbp
    ret
.size hipemu_switch, .-hipemu_switch
)");
struct Fiber { Ctx ctx; bool done = false; dim3 tid; int wave = 0, lane = 0; };

// one deferred atomicAdd: applied after the launch, in (block, program) order
struct AtomicRec { long long key; void* p; void (*apply)(void*, const void*); alignas(8) char val[8]; };
struct State {
  std::vector<Fiber> fibers;
  std::vector<WaveBuf> waves;
  std::vector<char*> stacks;
  Group block;
  Ctx sched;
  int cur = -1;
  long long block_key = 0;
  const std::function<void()>* body = nullptr;
  std::vector<AtomicRec> atomics;
};
inline State& st() { static thread_local State s; return s; }

}  // namespace hipemu

// threadIdx / blockIdx are plain globals rewritten by the scheduler before every resume
inline dim3& hipemu_threadIdx() { static thread_local dim3 v; return v; }
inline dim3& hipemu_blockIdx() { static thread_local dim3 v; return v; }
inline dim3& hipemu_blockDim() { static thread_local dim3 v; return v; }
inline dim3& hipemu_gridDim() { static thread_local dim3 v; return v; }
#define threadIdx (hipemu_threadIdx())
#define blockIdx (hipemu_blockIdx())
#define blockDim (hipemu_blockDim())
#define gridDim (hipemu_gridDim())

namespace hipemu {

inline void yield() {
  State& s = st();
  Fiber& f = s.fibers[s.cur];
  hipemu_switch(&f.ctx, &s.sched);
}
inline void barrier(Group& g) {
  unsigned gen = g.gen;
  if (++g.arrived == g.count) { g.arrived = 0; g.gen++; }
  else while (g.gen == gen) yield();
}
inline Fiber& me() { State& s = st(); return s.fibers[s.cur]; }
inline WaveBuf& mywave() { State& s = st(); return s.waves[s.fibers[s.cur].wave]; }

inline void fiber_entry() {
  State& s = st();
  (*s.body)();
  s.fibers[s.cur].done = true;
  hipemu_switch(&s.fibers[s.cur].ctx, &s.sched);
  abort();                                                   // a finished fiber is never resumed
}

inline std::vector<char>& dyn_smem_buf() { static thread_local std::vector<char> b; return b; }
inline void* dyn_smem() { return (void*)(((uintptr_t)dyn_smem_buf().data() + 63) & ~(uintptr_t)63); }

// all blocks [next, nblk) of one launch that this OS thread manages to claim
inline void run_blocks(dim3 grid, dim3 block, size_t shmem, const std::function<void()>& body, std::atomic<long long>& next, long long nblk) {
  State& s = st();
  if (dyn_smem_buf().size() < shmem + 64) dyn_smem_buf().resize(shmem + 64);
  const int nthr = (int)(block.x * block.y * block.z);
  const int nw = (nthr + WAVE - 1) / WAVE;
  while ((int)s.stacks.size() < nthr) {
    void* p = mmap(nullptr, STACK, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (p == MAP_FAILED) { perror("hipemu mmap"); abort(); }
    s.stacks.push_back((char*)p);
  }
  s.body = &body;
  hipemu_blockDim() = block;
  hipemu_gridDim() = grid;
  for (;;) {
    const long long lin = next.fetch_add(1);
    if (lin >= nblk) break;
    const unsigned bx = (unsigned)(lin % grid.x), by = (unsigned)((lin / grid.x) % grid.y), bz = (unsigned)(lin / ((long long)grid.x * grid.y));
    s.block_key = lin;
    s.fibers.assign(nthr, Fiber());
    s.waves.assign(nw, WaveBuf());
    s.block = Group();
    s.block.count = nthr;
    for (int t = 0; t < nthr; ++t) {
      Fiber& f = s.fibers[t];
      f.tid = dim3(t % block.x, (t / block.x) % block.y, t / (block.x * block.y));
      f.wave = t / WAVE;
      f.lane = t % WAVE;
      s.waves[f.wave].g.count++;
      // initial frame: 6 callee-saved slots + return address = fiber_entry; after the `ret` the stack
      // pointer is == 8 (mod 16), as at any function entry
      uintptr_t top = ((uintptr_t)s.stacks[t] + STACK) & ~(uintptr_t)15;
      void** sp = (void**)(top - 8) - 7;
      for (int q = 0; q < 6; ++q) sp[q] = nullptr;
      sp[6] = (void*)&fiber_entry;
      f.ctx.sp = sp;
    }
    int alive = nthr;
    while (alive > 0) {
      for (int t = 0; t < nthr; ++t) {
        Fiber& f = s.fibers[t];
        if (f.done) continue;
        s.cur = t;
        hipemu_threadIdx() = f.tid;
        hipemu_blockIdx() = dim3(bx, by, bz);
        hipemu_switch(&s.sched, &f.ctx);
        if (f.done) --alive;
      }
    }
  }
}

inline int max_threads() {
  static const int n = [] {
    const char* e = getenv("HIPEMU_THREADS");
    int v = e ? atoi(e) : (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    return v < 1 ? 1 : v;
  }();
  return n;
}

// [lo, hi) of the calling thread's TLS block of THIS library (where `__shared__` = static thread_local lives): atomics
// on LDS are block-local and applied at once, atomics on global memory are deferred (see launch)
inline void tls_range(uintptr_t& lo, uintptr_t& hi) {
  static thread_local uintptr_t r[2] = {0, 0};
  static thread_local bool have = false;
  if (!have) {
    static thread_local char probe;                               // lives in the TLS block we are looking for
    struct Q { uintptr_t probe, lo, hi; } q{(uintptr_t)&probe, 0, 0};
    dl_iterate_phdr([](struct dl_phdr_info* info, size_t, void* data) -> int {
      Q* q = (Q*)data;
      if (!info->dlpi_tls_data) return 0;
      for (int i = 0; i < info->dlpi_phnum; ++i)
        if (info->dlpi_phdr[i].p_type == PT_TLS) {
          const uintptr_t lo = (uintptr_t)info->dlpi_tls_data, hi = lo + info->dlpi_phdr[i].p_memsz;
          if (q->probe >= lo && q->probe < hi) { q->lo = lo; q->hi = hi; return 1; }
        }
      return 0;
    }, &q);
    r[0] = q.lo; r[1] = q.hi; have = true;
  }
  lo = r[0]; hi = r[1];
}
inline bool is_lds(const void* p) {
  uintptr_t lo, hi;
  tls_range(lo, hi);
  const uintptr_t a = (uintptr_t)p;
  if (a >= lo && a < hi) return true;
  const std::vector<char>& d = dyn_smem_buf();
  return !d.empty() && a >= (uintptr_t)d.data() && a < (uintptr_t)d.data() + d.size();
}

// persistent workers (their thread_local fiber stacks and LDS live across launches)
struct Job { dim3 grid, block; size_t shmem = 0; const std::function<void()>* body = nullptr; std::atomic<long long> next{0}; long long nblk = 0; };
struct Pool {
  std::mutex m;
  std::condition_variable cv_go, cv_done;
  std::vector<std::thread> th;
  std::vector<std::vector<AtomicRec>> logs;
  Job* job = nullptr;
  unsigned long long gen = 0;
  int want = 0, done = 0;
  void worker(int i) {
    unsigned long long seen = 0;
    for (;;) {
      Job* j;
      {
        std::unique_lock<std::mutex> lk(m);
        cv_go.wait(lk, [&] { return gen != seen && i < want; });
        seen = gen;
        j = job;
      }
      st().atomics.clear();
      run_blocks(j->grid, j->block, j->shmem, *j->body, j->next, j->nblk);
      {
        std::lock_guard<std::mutex> lk(m);
        logs[i].swap(st().atomics);
        if (++done == want) cv_done.notify_one();
      }
    }
  }
  // run `j` with `n` helper threads next to the caller
  void run(Job& j, int n) {
    {
      std::lock_guard<std::mutex> lk(m);
      while ((int)th.size() < n) { const int i = (int)th.size(); logs.emplace_back(); th.emplace_back([this, i] { worker(i); }); th.back().detach(); }
      for (auto& l : logs) l.clear();
      job = &j; want = n; done = 0; ++gen;
    }
    cv_go.notify_all();
    run_blocks(j.grid, j.block, j.shmem, *j.body, j.next, j.nblk);
    std::unique_lock<std::mutex> lk(m);
    cv_done.wait(lk, [&] { return done == want; });
    want = 0;
  }
};
inline Pool& pool() { static Pool* p = new Pool(); return *p; }      // leaked on purpose: workers are detached

// Devices and the dynamic-LDS opt-in, as on the GPU: the current device is the one hipSetDevice chose on this thread, else
// HIPEMU_DEVICE (default 0); a launch with more than 64 KiB of dynamic LDS runs only after hipFuncSetAttribute raised that
// function's limit to at least that much on the current device.  Otherwise it does not run and hipGetLastError reports it.
inline int& chosen_device() { static thread_local int d = -1; return d; }
inline int device() {
  if (chosen_device() >= 0) return chosen_device();
  const char* e = getenv("HIPEMU_DEVICE");
  return e ? atoi(e) : 0;
}
inline hipError_t& last_error() { static thread_local hipError_t e = hipSuccess; return e; }
struct Optins { std::mutex m; std::map<std::pair<int, const void*>, size_t> bytes; };      // (device, function) -> bytes
inline Optins& optins() { static Optins* o = new Optins(); return *o; }
inline size_t optin_bytes(int dev, const void* fn) {
  Optins& o = optins();
  std::lock_guard<std::mutex> lk(o.m);
  auto it = o.bytes.find({dev, fn});
  return it == o.bytes.end() ? 0 : it->second;
}

inline void launch(const void* fn, dim3 grid, dim3 block, size_t shmem, std::function<void()> body) {
  if (shmem > 65536 && optin_bytes(device(), fn) < shmem) { last_error() = hipErrorInvalidConfiguration; return; }
  Job j;
  j.grid = grid; j.block = block; j.shmem = shmem; j.body = &body;
  j.nblk = (long long)grid.x * grid.y * grid.z;
  const int nt = (int)std::min<long long>(max_threads(), j.nblk);
  std::vector<AtomicRec>& mine = st().atomics;
  mine.clear();
  if (nt > 1) {
    Pool& p = pool();
    p.run(j, nt - 1);
    for (int i = 0; i < nt - 1; ++i) mine.insert(mine.end(), p.logs[i].begin(), p.logs[i].end());
    // deferred global atomics: block order, program order inside a block (a block runs on one OS thread, so its
    // records are contiguous and ordered in that thread's log)
    std::stable_sort(mine.begin(), mine.end(), [](const AtomicRec& a, const AtomicRec& b) { return a.key < b.key; });
  } else {
    run_blocks(grid, block, shmem, body, j.next, j.nblk);
  }
  for (const AtomicRec& r : mine) r.apply(r.p, r.val);
  mine.clear();
}

}  // namespace hipemu

#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) \
  hipemu::launch(reinterpret_cast<const void*>(&kernel), (grid), (block), (size_t)(shmem), [=]() { kernel(__VA_ARGS__); })
static inline hipError_t hipGetLastError() { const hipError_t e = hipemu::last_error(); hipemu::last_error() = hipSuccess; return e; }
static inline hipError_t hipPeekAtLastError() { return hipemu::last_error(); }
static inline hipError_t hipSetDevice(int d) { hipemu::chosen_device() = d; return hipSuccess; }
static inline hipError_t hipGetDevice(int* d) { *d = hipemu::device(); return hipSuccess; }
static inline hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t, int) {
  const char* e = getenv("HIPEMU_MAX_LDS");
  *v = e ? atoi(e) : 160 * 1024;
  return hipSuccess;
}
static inline hipError_t hipFuncSetAttribute(const void* fn, hipFuncAttribute, int bytes) {
  hipemu::Optins& o = hipemu::optins();
  std::lock_guard<std::mutex> lk(o.m);
  o.bytes[{hipemu::device(), fn}] = (size_t)bytes;
  return hipSuccess;
}
#define LEMO_DYN_SMEM(var) float* var = (float*)hipemu::dyn_smem()

// ---- synchronisation & cross-lane ---------------------------------------------------------
static inline void __syncthreads() { hipemu::barrier(hipemu::st().block); }
static inline void __builtin_amdgcn_s_barrier() { hipemu::barrier(hipemu::st().block); }
static inline void __threadfence() {}
static inline void __threadfence_block() {}

template <typename T>
static inline T hipemu_exchange(T v, int src_lane) {
  static_assert(sizeof(T) <= 8, "exchange <= 8 bytes");
  hipemu::WaveBuf& w = hipemu::mywave();
  const int lane = hipemu::me().lane;
  unsigned long long raw = 0;
  memcpy(&raw, &v, sizeof(T));
  w.u[lane] = raw;
  hipemu::barrier(w.g);
  unsigned long long got = (src_lane >= 0 && src_lane < w.g.count) ? w.u[src_lane] : raw;
  hipemu::barrier(w.g);
  T out;
  memcpy(&out, &got, sizeof(T));
  return out;
}
template <typename T> static inline T __shfl_xor(T v, int mask, int width = 64) {
  const int lane = hipemu::me().lane;
  const int src = lane ^ mask;
  return hipemu_exchange(v, (src / width == lane / width) ? src : lane);
}
template <typename T> static inline T __shfl_down(T v, unsigned d, int width = 64) {
  const int lane = hipemu::me().lane;
  const int src = lane + (int)d;
  return hipemu_exchange(v, (src / width == lane / width) ? src : lane);
}
template <typename T> static inline T __shfl_up(T v, unsigned d, int width = 64) {
  const int lane = hipemu::me().lane;
  const int src = lane - (int)d;
  return hipemu_exchange(v, (src >= 0 && src / width == lane / width) ? src : lane);
}
template <typename T> static inline T __shfl(T v, int src, int width = 64) {
  const int lane = hipemu::me().lane;
  return hipemu_exchange(v, (lane / width) * width + (src % width));
}
static inline unsigned long long __ballot(int pred) {
  hipemu::WaveBuf& w = hipemu::mywave();
  const int lane = hipemu::me().lane;
  w.u[lane] = pred ? 1ull : 0ull;
  hipemu::barrier(w.g);
  unsigned long long m = 0;
  for (int i = 0; i < w.g.count; ++i) m |= (w.u[i] & 1ull) << i;
  hipemu::barrier(w.g);
  return m;
}

// DPP row operations used by the reductions (common.hpp): quad_perm, row_mirror, row_half_mirror, row_ror
static inline int __builtin_amdgcn_update_dpp(int, int src, int ctrl, int, int, bool) {
  const int lane = hipemu::me().lane;
  int from = lane;
  if (ctrl >= 0 && ctrl <= 0xFF) from = (lane & ~3) | ((ctrl >> (2 * (lane & 3))) & 3);
  else if (ctrl == 0x140) from = (lane & ~15) | (15 - (lane & 15));
  else if (ctrl == 0x141) from = (lane & ~7) | (7 - (lane & 7));
  else if (ctrl > 0x120 && ctrl <= 0x12F) from = (lane & ~15) | ((lane - (ctrl - 0x120)) & 15);
  else abort();
  return hipemu_exchange(src, from);
}
static inline int __builtin_amdgcn_readlane(int v, int lane) { return hipemu_exchange(v, lane); }
// gfx950 v_permlane32_swap: the upper 32 lanes of the first operand trade places with the lower 32 lanes of the second;
// returns {new first, new second}
typedef unsigned hipemu_u32x2s __attribute__((ext_vector_type(2)));
static inline hipemu_u32x2s __builtin_amdgcn_permlane32_swap(unsigned a, unsigned b, bool, bool) {
  const int lane = hipemu::me().lane;
  const unsigned a_from = hipemu_exchange(a, lane ^ 32), b_from = hipemu_exchange(b, lane ^ 32);
  hipemu_u32x2s r;
  r[0] = lane < 32 ? a : b_from;         // a[32..63] <- b[0..31]
  r[1] = lane < 32 ? a_from : b;         // b[0..31] <- a[32..63]
  return r;
}

// ---- MFMA (f32 in / f32 acc) ----------------------------------------------------------------
typedef float hipemu_f32x16 __attribute__((ext_vector_type(16)));
typedef float hipemu_f32x4 __attribute__((ext_vector_type(4)));

static inline hipemu_f32x16 __builtin_amdgcn_mfma_f32_32x32x2f32(float a, float b, hipemu_f32x16 c, int, int, int) {
  hipemu::WaveBuf& w = hipemu::mywave();
  const int l = hipemu::me().lane;
  w.a[l] = a; w.b[l] = b;
  hipemu::barrier(w.g);
  hipemu_f32x16 d;
  const int col = l & 31;
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
    float acc = c[r];
    for (int k = 0; k < 2; ++k) acc = fmaf(w.a[row + 32 * k], w.b[col + 32 * k], acc);
    d[r] = acc;
  }
  hipemu::barrier(w.g);
  return d;
}
static inline hipemu_f32x4 __builtin_amdgcn_mfma_f32_16x16x4f32(float a, float b, hipemu_f32x4 c, int, int, int) {
  hipemu::WaveBuf& w = hipemu::mywave();
  const int l = hipemu::me().lane;
  w.a[l] = a; w.b[l] = b;
  hipemu::barrier(w.g);
  hipemu_f32x4 d;
  const int col = l & 15;
  for (int r = 0; r < 4; ++r) {
    const int row = 4 * (l >> 4) + r;
    float acc = c[r];
    for (int k = 0; k < 4; ++k) acc = fmaf(w.a[row + 16 * k], w.b[col + 16 * k], acc);
    d[r] = acc;
  }
  hipemu::barrier(w.g);
  return d;
}

// gfx950 bf16 MFMA: A[i = l&31][k = 8*(l>>5)+e], B[k][j = l&31], C/D as the f32 32x32 form; the 16
// products of one instruction are exact and summed before the single fp32 rounding
typedef __bf16 hipemu_bf16x8 __attribute__((ext_vector_type(8)));
static inline hipemu_f32x16 __builtin_amdgcn_mfma_f32_32x32x16_bf16(hipemu_bf16x8 a, hipemu_bf16x8 b, hipemu_f32x16 c, int, int, int) {
  hipemu::WaveBuf& w = hipemu::mywave();
  const int l = hipemu::me().lane;
  for (int e = 0; e < 8; ++e) { w.a8[l][e] = (float)a[e]; w.b8[l][e] = (float)b[e]; }
  hipemu::barrier(w.g);
  hipemu_f32x16 d;
  const int col = l & 31;
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
    double acc = c[r];
    for (int hh = 0; hh < 2; ++hh)
      for (int e = 0; e < 8; ++e) acc += (double)w.a8[row + 32 * hh][e] * (double)w.b8[col + 32 * hh][e];
    d[r] = (float)acc;
  }
  hipemu::barrier(w.g);
  return d;
}

// gfx950 f16 MFMA: same operand / result lane maps as the bf16 form; products of two f16 values are exact in fp32 terms,
// summed in double here and rounded once per instruction
typedef _Float16 hipemu_f16x8 __attribute__((ext_vector_type(8)));
static inline hipemu_f32x16 __builtin_amdgcn_mfma_f32_32x32x16_f16(hipemu_f16x8 a, hipemu_f16x8 b, hipemu_f32x16 c, int, int, int) {
  hipemu::WaveBuf& w = hipemu::mywave();
  const int l = hipemu::me().lane;
  for (int e = 0; e < 8; ++e) { w.a8[l][e] = (float)a[e]; w.b8[l][e] = (float)b[e]; }
  hipemu::barrier(w.g);
  hipemu_f32x16 d;
  const int col = l & 31;
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
    double acc = c[r];
    for (int hh = 0; hh < 2; ++hh)
      for (int e = 0; e < 8; ++e) acc += (double)w.a8[row + 32 * hh][e] * (double)w.b8[col + 32 * hh][e];
    d[r] = (float)acc;
  }
  hipemu::barrier(w.g);
  return d;
}

// gfx950 v_mfma_f32_16x16x32_f16: A[i = l&15][k = 8*(l>>4)+e], B[k][j = l&15], D[i = 4*(l>>4)+r][j = l&15] (r = 0..3); the 32
// products of one instruction are exact, summed in double here and rounded once
static inline hipemu_f32x4 __builtin_amdgcn_mfma_f32_16x16x32_f16(hipemu_f16x8 a, hipemu_f16x8 b, hipemu_f32x4 c, int, int, int) {
  hipemu::WaveBuf& w = hipemu::mywave();
  const int l = hipemu::me().lane;
  for (int e = 0; e < 8; ++e) { w.a8[l][e] = (float)a[e]; w.b8[l][e] = (float)b[e]; }
  hipemu::barrier(w.g);
  hipemu_f32x4 d;
  const int col = l & 15;
  for (int r = 0; r < 4; ++r) {
    const int row = 4 * (l >> 4) + r;
    double acc = c[r];
    for (int q = 0; q < 4; ++q)
      for (int e = 0; e < 8; ++e) acc += (double)w.a8[row + 16 * q][e] * (double)w.b8[col + 16 * q][e];
    d[r] = (float)acc;
  }
  hipemu::barrier(w.g);
  return d;
}

// ---- atomics: atomicAdd on GLOBAL memory is deferred to the end of the launch (see hipemu::launch); its return value is
// NOT the old value (no kernel uses it).  Integer fetch-adds whose result IS used (last-block detection) are real atomics.
template <typename T> static void hipemu_apply_add(void* p, const void* v) { T a; memcpy(&a, v, sizeof(T)); *(T*)p = *(T*)p + a; }
template <typename T> static inline T atomicAdd(T* p, T v) {
  static_assert(sizeof(T) <= 8, "atomicAdd operand <= 8 bytes");
  if (hipemu::is_lds(p)) { T o = *p; *p = o + v; return o; }     // LDS: block-local, one OS thread
  hipemu::State& s = hipemu::st();
  hipemu::AtomicRec r;
  r.key = s.block_key; r.p = (void*)p; r.apply = &hipemu_apply_add<T>;
  memcpy(r.val, &v, sizeof(T));
  s.atomics.push_back(r);
  return T();
}
static inline float atomicAdd(float* p, double v) { return atomicAdd(p, (float)v); }
// atomicMax on unsigned (the kernels use it on the bit patterns of non-negative floats): deferred like atomicAdd, order-independent
static void hipemu_apply_umax(void* p, const void* v) { unsigned a; memcpy(&a, v, 4); if (a > *(unsigned*)p) *(unsigned*)p = a; }
static inline unsigned atomicMax(unsigned* p, unsigned v) {
  if (hipemu::is_lds(p)) { unsigned o = *p; if (v > o) *p = v; return o; }
  hipemu::State& s = hipemu::st();
  hipemu::AtomicRec r;
  r.key = s.block_key; r.p = (void*)p; r.apply = &hipemu_apply_umax;
  memcpy(r.val, &v, 4);
  s.atomics.push_back(r);
  return 0u;
}

// ---- buffer resources / cache-policy loads & stores / scoped atomics (plain memory on the host) ------------
struct hipDeviceProp_t { int multiProcessorCount; };
// (workgroups run one after another here: multi-layer chains cannot make progress -- the CPU tests use n = 1)
static inline hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) { p->multiProcessorCount = 1 << 20; return hipSuccess; }
struct hipemu_rsrc { char* p; };
typedef hipemu_rsrc __amdgpu_buffer_rsrc_t;
typedef unsigned hipemu_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned hipemu_u32x2 __attribute__((ext_vector_type(2)));
static inline __amdgpu_buffer_rsrc_t __builtin_amdgcn_make_buffer_rsrc(void* p, short, int, int) { return hipemu_rsrc{(char*)p}; }
static inline hipemu_u32x4 __builtin_amdgcn_raw_buffer_load_b128(__amdgpu_buffer_rsrc_t r, int voff, int soff, int) {
  hipemu_u32x4 v; memcpy(&v, r.p + voff + soff, 16); return v;
}
static inline unsigned __builtin_amdgcn_raw_buffer_load_b32(__amdgpu_buffer_rsrc_t r, int voff, int soff, int) {
  unsigned v; memcpy(&v, r.p + voff + soff, 4); return v;
}
static inline void __builtin_amdgcn_raw_buffer_store_b128(hipemu_u32x4 v, __amdgpu_buffer_rsrc_t r, int voff, int soff, int) { memcpy(r.p + voff + soff, &v, 16); }
static inline void __builtin_amdgcn_raw_buffer_store_b64(hipemu_u32x2 v, __amdgpu_buffer_rsrc_t r, int voff, int soff, int) { memcpy(r.p + voff + soff, &v, 8); }
static inline void __builtin_amdgcn_raw_buffer_store_b32(unsigned v, __amdgpu_buffer_rsrc_t r, int voff, int soff, int) { memcpy(r.p + voff + soff, &v, 4); }
#define __HIP_MEMORY_SCOPE_AGENT 4
#define __hip_atomic_load(p, order, scope) __atomic_load_n((p), __ATOMIC_SEQ_CST)
#define __hip_atomic_store(p, v, order, scope) __atomic_store_n((p), (v), __ATOMIC_SEQ_CST)
template <typename T> static inline T hipemu_fetch_add(T* p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
#define __hip_atomic_fetch_add(p, v, order, scope) hipemu_fetch_add((p), (v))
static inline void __builtin_amdgcn_s_sleep(int) {}
static inline void __builtin_amdgcn_s_waitcnt(int) {}

static inline void __builtin_amdgcn_wave_barrier() { hipemu::barrier(hipemu::mywave().g); }
static inline void __builtin_amdgcn_sched_barrier(int) {}
static inline void __builtin_amdgcn_sched_group_barrier(int, int, int) {}
static inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
// only ever applied to wave-uniform values in the kernels
static inline int __builtin_amdgcn_readfirstlane(int v) { return v; }
static inline unsigned __builtin_amdgcn_s_getreg(int) { return 0u; }
static inline void __builtin_amdgcn_s_setprio(int) {}
static inline unsigned long long __builtin_amdgcn_s_memtime() { return 0ull; }

// ---- math -----------------------------------------------------------------------------------
static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
static inline float __fdividef(float a, float b) { return a / b; }
#define __expf(x) expf(x)
static inline float __frcp_rn(float x) { return 1.0f / x; }
static inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
static inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
static inline unsigned __float_as_uint(float f) { unsigned i; memcpy(&i, &f, 4); return i; }
static inline float __uint_as_float(unsigned i) { float f; memcpy(&f, &i, 4); return f; }
using std::max;
using std::min;
