// Cost of the step group's cross-stream event chain and of a timing event pair, per event-creation flag.
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tools/probe/event_hops tools/probe/event_hops.hip && tools/probe/event_hops [rounds] [kernel_us]
//
// Two streams, one busy-wait kernel of ~0.5 ms on 64 workgroups of 64 lanes (the shape of the merged step dispatch: a launch that lasts as long as one
// serial chain and leaves the chip empty).  Per flag set, `rounds` rounds each, wall time per round minus the wall time per round of the bare launches:
//   chain   the chain of DESIGN 31.4: launch on s0, record `done` on s0, s1 waits for it; next round: record `join` on s1, s0 waits for it, launch
//   quiet   the same without the join (record `done`, s1 waits): what a continuing round of a "quiet_streams" group queues
//   pair    an event pair recorded around the launch on s0 (a ring of 128 pairs, as in the library)
// `done` and `join` are one event each, recorded again every round, as in the library.  The host only enqueues: one device synchronisation per series.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)

constexpr int WGS = 64, LANES = 64, RING = 128;

// spins on the constant-rate wall clock for `ticks`; the iteration cap ends the kernel whatever the clock does
__global__ __launch_bounds__(LANES) void k_busy(long long ticks, long long* out) {
  const long long t0 = wall_clock64();
  long long t = t0;
  for (int i = 0; i < (1 << 22) && t - t0 < ticks; i++) { __builtin_amdgcn_s_sleep(8); t = wall_clock64(); }
  if (threadIdx.x == 0) out[blockIdx.x] = t - t0;      // out has WGS words
}

struct Ctx { hipStream_t s0, s1; long long ticks; long long* out; int rounds; };
static void launch(const Ctx& c) { hipLaunchKernelGGL(k_busy, dim3(WGS), dim3(LANES), 0, c.s0, c.ticks, c.out); CHK(hipGetLastError()); }

template <class F> static double per_round_us(const Ctx& c, F body) {
  for (int i = 0; i < 20; i++) body(i);      // warm-up: code object, queues, signal pools
  CHK(hipDeviceSynchronize());
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < c.rounds; i++) body(i);
  CHK(hipDeviceSynchronize());
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / c.rounds;
}

int main(int argc, char** argv) {
  Ctx c;
  c.rounds = argc > 1 ? std::atoi(argv[1]) : 300;
  const double kernel_us = argc > 2 ? std::atof(argv[2]) : 500.0;
  if (c.rounds < 1 || c.rounds > 100000 || kernel_us < 1.0 || kernel_us > 5000.0) { std::fprintf(stderr, "usage: event_hops [rounds 1..100000] [kernel_us 1..5000]\n"); return 2; }
  CHK(hipSetDevice(0));
  int khz = 0;
  CHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0));
  if (khz <= 0) khz = 100000;
  c.ticks = (long long)(kernel_us * 1e-3 * khz);
  CHK(hipStreamCreateWithFlags(&c.s0, hipStreamNonBlocking));
  CHK(hipStreamCreateWithFlags(&c.s1, hipStreamNonBlocking));
  CHK(hipMalloc(&c.out, WGS * sizeof(long long)));
  const double bare = per_round_us(c, [&](int) { launch(c); });
  const double bare2 = per_round_us(c, [&](int) { launch(c); });
  std::printf("wall clock %d kHz, kernel %lld ticks, %d rounds; bare launches back to back on s0: %.2f us per round (second series %.2f)\n", khz, c.ticks, c.rounds, bare, bare2);
  struct Flags { const char* name; unsigned flags; bool chain; };
  const Flags sets[] = {
    {"default", hipEventDefault, true},
    {"DisableTiming", hipEventDisableTiming, true},
    {"DisableTiming|DisableSystemFence", hipEventDisableTiming | hipEventDisableSystemFence, true},
    {"ReleaseToDevice", hipEventReleaseToDevice, true},
    {"DisableSystemFence (timing on)", hipEventDisableSystemFence, false},
  };
  std::printf("%-36s %12s %12s %12s %14s\n", "event flags", "chain us", "quiet us", "pair us", "pair reads ms");
  for (const Flags& f : sets) {
    hipEvent_t done, join, r0[RING], r1[RING];
    CHK(hipEventCreateWithFlags(&done, f.flags));
    CHK(hipEventCreateWithFlags(&join, f.flags));
    for (int i = 0; i < RING; i++) { CHK(hipEventCreateWithFlags(&r0[i], f.flags)); CHK(hipEventCreateWithFlags(&r1[i], f.flags)); }
    double chain = 0.0, quiet = 0.0;
    if (f.chain) {
      // s1 has a `done` to wait for from the first round on
      CHK(hipEventRecord(done, c.s0)); CHK(hipStreamWaitEvent(c.s1, done, 0));
      chain = per_round_us(c, [&](int) {
        CHK(hipEventRecord(join, c.s1)); CHK(hipStreamWaitEvent(c.s0, join, 0));
        launch(c);
        CHK(hipEventRecord(done, c.s0)); CHK(hipStreamWaitEvent(c.s1, done, 0));
      }) - bare;
      quiet = per_round_us(c, [&](int) {
        launch(c);
        CHK(hipEventRecord(done, c.s0)); CHK(hipStreamWaitEvent(c.s1, done, 0));
      }) - bare;
    }
    const double pair = per_round_us(c, [&](int i) {
      CHK(hipEventRecord(r0[i % RING], c.s0));
      launch(c);
      CHK(hipEventRecord(r1[i % RING], c.s0));
    }) - bare;
    float ms = -1.0f;      // what the last pair reports for the kernel (events without timing: not readable)
    if (!(f.flags & hipEventDisableTiming)) CHK(hipEventElapsedTime(&ms, r0[(c.rounds - 1) % RING], r1[(c.rounds - 1) % RING]));
    if (f.chain) std::printf("%-36s %12.2f %12.2f %12.2f %14.4f\n", f.name, chain, quiet, pair, ms);
    else std::printf("%-36s %12s %12s %12.2f %14.4f\n", f.name, "-", "-", pair, ms);
    CHK(hipEventDestroy(done)); CHK(hipEventDestroy(join));
    for (int i = 0; i < RING; i++) { CHK(hipEventDestroy(r0[i])); CHK(hipEventDestroy(r1[i])); }
  }
  long long host[WGS];
  CHK(hipMemcpy(host, c.out, sizeof host, hipMemcpyDeviceToHost));
  std::printf("last kernel: workgroup 0 spun for %lld ticks\n", host[0]);
  CHK(hipFree(c.out)); CHK(hipStreamDestroy(c.s0)); CHK(hipStreamDestroy(c.s1));
  return 0;
}
