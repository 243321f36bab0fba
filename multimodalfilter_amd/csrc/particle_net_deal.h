// The dealing of the run-consuming dynamics launch (particle_net.hip, RUNS): which real tiles a workgroup computes.
// A trajectory with n_runs runs holds c = ceil(n_runs / TILE) real tiles; the real tiles of a launch, trajectory-major, form
// a dense list of P[N] entries (P: the exclusive prefix sum of c), and dense index k goes to workgroup k mod G -- one tile
// at a time, round-robin, so two workgroups differ by at most one tile and the tiles of one trajectory (which share its
// expansion weight) land on different workgroups.  Pure functions, compiled by both sides: the kernel builds P with a
// block-wide scan and calls these per entry, mmf_pf_dedup_deal (the host entry point the tests read) calls the same ones.
#pragma once

#if defined(__HIPCC__)
#define MMF_DEAL_HD __host__ __device__ __forceinline__
#else
#define MMF_DEAL_HD inline
#endif

namespace mmf_deal {

// what a run table can hold: 1 .. M runs
MMF_DEAL_HD int clamp_runs(int n_runs, int M) { return n_runs < 1 ? 1 : (n_runs > M ? M : n_runs); }

// real tiles of a trajectory: 1 .. M / tile
MMF_DEAL_HD int tiles_of_runs(int n_runs, int M, int tile) { return (clamp_runs(n_runs, M) + tile - 1) / tile; }

// entries of workgroup b's list: dense indices b, b + G, .. below total
MMF_DEAL_HD int list_length(int total, int grid, int b) { return b < total ? (total - b + grid - 1) / grid : 0; }

// first step of find_traj for n_traj trajectories: the largest power of two below n_traj (0 for one trajectory)
MMF_DEAL_HD int search_top(int n_traj) {
  int top = 0;
  for (int s = 1; s < n_traj; s <<= 1) top = s;
  return top;
}

// max{n in [0, n_traj) : P[n] <= k} for k >= P[0] = 0: a descent with a fixed trip count (top: a power of two with
// 2 top >= n_traj, or 0); every index it reads is below n_traj
MMF_DEAL_HD int find_traj(const int* P, int n_traj, int k, int top) {
  int pos = 0;
  for (int s = top; s > 0; s >>= 1) {
    const int probe = pos + s;
    if (probe < n_traj && P[probe] <= k) pos = probe;
  }
  return pos;
}

// tile q of trajectory traj as the launch's tile number q' n_traj + traj, q = (q' + traj) mod tiles_per_traj (run_tile's
// rotation, inverted)
MMF_DEAL_HD int tile_number(int traj, int q, int n_traj, int tiles_per_traj) {
  int qr = (q - traj % tiles_per_traj) % tiles_per_traj;
  qr = qr < 0 ? qr + tiles_per_traj : qr;
  return qr * n_traj + traj;
}

// entry i of workgroup b's list (i < list_length): dense index k = b + i G -> (traj, q) -> tile number.  traj and q are
// clamped to what the launch holds, so a P that is no prefix sum still gives a tile below n_traj tiles_per_traj.
MMF_DEAL_HD int list_entry(const int* P, int n_traj, int tiles_per_traj, int grid, int b, int i, int top) {
  const int k = b + i * grid;
  const int traj = find_traj(P, n_traj, k, top);
  int q = k - P[traj];
  q = q < 0 ? 0 : (q >= tiles_per_traj ? tiles_per_traj - 1 : q);
  return tile_number(traj, q, n_traj, tiles_per_traj);
}

}  // namespace mmf_deal
