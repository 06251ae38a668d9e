// Loop level of the two training engines (ae_train_engine.hip, prior_train_engine.hip): the batch-assembly kernels that build a
// step's batch from a device-resident dataset, the step cursor and loss log of an epoch, and the step counter of a training-state
// blob (train_epoch_kernels.hip).
#pragma once
#include "kernels.hpp"
#include "engine_host.hpp"

namespace lemo {

// What both training engines keep next to their networks: the replay state of a step and of an epoch's step, and the two
// workspace blocks the loop level reads (ctr: Adam's counter + the epoch block below; losses: the last step's loss terms)
struct TrainReplay {
  int use_graph = 0, loaded = 0;
  hipGraphExec_t exec = nullptr;                        // one training step
  hipGraphExec_t exec_ep[2] = {nullptr, nullptr};       // one step of an epoch (assemble, step, log): [0] evaluation, [1] training
  float *ctr = nullptr, *losses = nullptr;
  void destroy_graphs() { lemo::destroy_graphs(&exec, 1); lemo::destroy_graphs(exec_ep, 2); }
};

// What the kernels of an epoch read from DEVICE memory: the engine keeps one EpochBlock in the spare floats of its `ctr` block
// (floats EP_BLOCK_OFF .. 63; Adam's counter uses 0 .. 2).  ep_begin writes it once per lemo_*train_epoch call, so a captured
// step graph carries none of the caller's pointers and is replayed n_steps times with no host patching: the assembly kernel and
// the log write read `cursor`, ep_end (the step's last kernel) advances it.
#define EP_BLOCK_OFF 16
struct EpochBlock {
  const float* data;          // AE [n_clips][4][H - 2][W - 16]; smoothness [n_clips][1][H - 2][W - 15]
  const int* idx;             // [n_steps][bs] clip of every batch slot
  const int* marker_ids;      // recipe LEMO_MASK_RANDOM: [n_steps][bs][6], -1 = unused
  const float* masks;         // recipe LEMO_MASK_PROX: [n_masks][67][mask_len]
  const int* mask_idx;        // recipe LEMO_MASK_PROX: [n_steps][bs]
  float* log;                 // [n_steps][nloss]
  int n_clips, n_masks, mask_len, n_steps, recipe, cursor;
};
static_assert(sizeof(EpochBlock) <= (64 - EP_BLOCK_OFF) * sizeof(float), "the epoch block lives in the spare floats of ctr");
static inline EpochBlock* ep_block(float* ctr) { return reinterpret_cast<EpochBlock*>(ctr + EP_BLOCK_OFF); }

int ep_begin(const EpochBlock& B, EpochBlock* dev, hipStream_t s);                                  // *dev = B, cursor = 0
int ep_end(EpochBlock* dev, const float* losses, int nloss, hipStream_t s);                         // log row `cursor` <- losses; ++cursor
// step `dev->cursor` (dev != null) or `step` of B: the AE's batch into the engine's buffers (x8: CG8P interior, channels 0 .. 3 of
// each image, images cs floats apart; ybuf [bs][H][W]) or in the API layout (x [bs][4][H][W], y [bs][H][W])
int aet_assemble(const EpochBlock& B, const EpochBlock* dev, int step, float* x8, size_t cs, float* ybuf, int bs, int H, int W, hipStream_t s);
int aet_assemble_api(const EpochBlock& B, int step, float* x, float* y, int bs, int H, int W, hipStream_t s);
// the smoothness prior's batch x [bs][H][W] (the engine's xin has the API layout)
int sp_assemble(const EpochBlock& B, const EpochBlock* dev, int step, float* x, int bs, int H, int W, hipStream_t s);
// Adam's step counter (ctr[0], an int) <-> two floats of a state blob: {step mod 2^24, step div 2^24}, both exact in fp32
int train_step_counter(float* ctr, float* blob, bool save, hipStream_t s);

}  // namespace lemo
