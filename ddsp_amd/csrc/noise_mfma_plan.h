// How noise_mfma65_kernel's tiles are dealt to its persistent blocks (filtered_noise_mfma.hip): plain host C++, no HIP, so that
// tests/test_noise_mfma_plan.py can compile and check it on any machine.
//
// A batch row is `frames` staged frames of 64 samples long (its outputs z[0 .. N + start) in whole frames).  A tile stages 32
// of them.  Cut alone, a tile spends its first two staged frames on history - the 128 taps reach 127 samples back - and has 30
// output frames; a tile that CONTINUES where the block's previous tile ended is handed that history's contribution (the carry
// of the previous tile's last pair) and has 32.  So every block gets RUNS of `run_len` consecutive tiles of one row: 30 + 32
// (run_len - 1) output frames for run_len ticks.  A row is cut into `runs_per_row` runs, run r starting at output frame r *
// run_frames; all runs have run_len tiles, and those of a row's last run that lie past its end cost next to nothing.  Runs go
// round-robin to min(n_runs, slots) blocks, a block walks its runs one after the other; the rows' LAST runs, the short ones,
// come last in that order (run ids n_whole ..), so that they top up the blocks with one whole run less.
//
// The plan depends on the batch size - and the kernel's results do not: every output sample is formed by the same additions in
// the same order wherever the tile boundaries fall (see the FIR wavefronts), so a row run alone equals the row in any batch.
#pragma once

namespace ddsp {

constexpr int kMfPlanTileFrames = 32;          // staged frames per tile (kMfRows)
constexpr int kMfPlanHistory = 2;              // of which history in a run's first tile
constexpr int kMfPlanTick = 4;                 // what a tick costs whatever its tile holds (barrier, set-up), in staged frames

struct MfRunPlan {
  int frames;          // staged frames of 64 samples a row's outputs take: ceil((F * frame_size + start) / 64)
  int run_len;         // tiles per run
  int run_frames;      // output frames per run: 30 + 32 (run_len - 1)
  int runs_per_row;
  int n_runs;          // B * runs_per_row
  int n_whole;         // B * (runs_per_row - 1): the runs before the rows' last ones
  int grid;            // blocks: min(n_runs, slots)
  int ticks;           // tiles of the busiest block: run_len * ceil(n_runs / grid)
  long cost;           // the busiest block's work in staged frames (what the plan minimises)
};

inline int mf_run_frames(int run_len) { return kMfPlanTileFrames * run_len - kMfPlanHistory; }

// what a run of `len` tiles costs when only its first `out_frames` output frames exist
inline long mf_run_cost(int len, int out_frames) {
  long c = (long)kMfPlanTick * len;
  int staged = out_frames + kMfPlanHistory;
  for (int j = 0; j < len && staged > 0; ++j, staged -= kMfPlanTileFrames) c += staged < kMfPlanTileFrames ? staged : kMfPlanTileFrames;
  return c;
}

// B rows of F frames of frame_size samples (a multiple of 64), outputs delayed by `start`; slots = blocks the chip holds at once.
// Among all run lengths the one whose busiest block has the least work; among equals the longest (fewest runs: least history
// recomputed).  Wherever the tiles fit the slots that is one tile per block (run_len = 1).
inline MfRunPlan plan_noise_mfma_runs(int B, int F, int frame_size, int start, int slots) {
  MfRunPlan best{};
  const long samples = (long)F * frame_size + start;
  const int frames = (int)((samples + 63) / 64);
  const int max_len = (frames + kMfPlanHistory + kMfPlanTileFrames - 1) / kMfPlanTileFrames;     // one run takes the whole row
  int last_rpr = 0;
  for (int len = 1; len <= (max_len > 1 ? max_len : 1); ++len) {
    const int rf = mf_run_frames(len);
    const int rpr = (frames + rf - 1) / rf;
    if (rpr == last_rpr) continue;               // the same cut with longer runs: only more tiles past the end
    last_rpr = rpr;
    const long n_runs = (long)B * rpr, n_whole = (long)B * (rpr - 1);
    const long grid = n_runs < slots ? n_runs : slots;
    const long whole_cost = mf_run_cost(len, rf), last_cost = mf_run_cost(len, frames - (rpr - 1) * rf);
    long cost = 0;
    for (long i = 0; i < grid; ++i) {
      const long whole = n_whole > i ? (n_whole - i + grid - 1) / grid : 0;
      const long all = (n_runs - i + grid - 1) / grid;
      const long c = whole * whole_cost + (all - whole) * last_cost;
      if (c > cost) cost = c;
    }
    if (best.run_len == 0 || cost <= best.cost) {             // (the runs get fewer as they get longer)
      best.frames = frames; best.run_len = len; best.run_frames = rf; best.runs_per_row = rpr;
      best.n_runs = (int)n_runs; best.n_whole = (int)n_whole; best.grid = (int)grid;
      best.ticks = (int)(len * ((n_runs + grid - 1) / grid)); best.cost = cost;
    }
  }
  return best;
}

// Run id -> (batch row, run of the row), as the kernel does it.
inline void mf_plan_run(const MfRunPlan& p, int run, int* b, int* r) {
  if (run >= p.n_whole) { *b = run - p.n_whole; *r = p.runs_per_row - 1; }
  else { *b = run / (p.runs_per_row - 1); *r = run % (p.runs_per_row - 1); }
}
// Tile j of run r of a row: its first staged frame (-2: the start of the row), its first output frame, and whether it continues.
struct MfPlanTile { int staged, first_out, cont; };
inline MfPlanTile mf_plan_tile(const MfRunPlan& p, int r, int j) {
  const int staged = r * p.run_frames + kMfPlanTileFrames * j - kMfPlanHistory;
  return MfPlanTile{staged, j ? staged : staged + kMfPlanHistory, j != 0};
}

}  // namespace ddsp
