// somar_amd/csrc/tuning.h -- the execution-path switches of the library, one value per solver.
// Tuning::from_env() is the only reader of the SOMAR_* tuning variables: a PressureSolver, AMRSolver or LepticSolver
// calls it once when it is created, keeps the value for its life and hands the same value to its parts (level
// solvers, coarsened-fine levels, the agglomerated tail -- the tail's copy has graph_cells = 0, its only difference),
// so one user-visible solver has one set of values whatever happens to the environment afterwards.  Every alternative
// path computes the same values; defaults are the fast paths.
// A field carries what its variable says, in the variable's own sense (SOMAR_NO_x: 1 = x is off).
#pragma once

namespace somar {

struct Tuning {
    // ---- which kernels a level runs ----
    long long fused_min_cells = 262144;   // SOMAR_FUSED_MIN_CELLS: levels at least this big run the fused red+black sweep (tests: 0)
    long long march_min_cells = 262144;   // SOMAR_MARCH_MIN_CELLS: ... and the k-marching operator / residual / 19-point kernels (unset: fused_min_cells)
    long long fused_rows = 16;            // SOMAR_FUSED_ROWS: region rows per workgroup of the fused 7-point sweep, 16 or 8
    long long full_rows = 8;              // SOMAR_FULL_ROWS: region rows per workgroup of the 19-point marching kernels, 8 or 6
    // ---- tile columns of the marching kernels (Level::build_march_tiles) ----
    long long no_balanced_tiles = 0;      // SOMAR_NO_BALANCED_TILES: plain 124-wide columns instead of equal ones
    long long no_narrow_tiles = 0;        // SOMAR_NO_NARROW_TILES: equal columns only, no narrow lane classes
    long long narrow_7pt = -1;            // SOMAR_NARROW_7PT: lane classes for the 7-point kernels never (0) / always (1); unset (-1): on uniform-metric depths
    long long no_lean_tiles = 0;          // SOMAR_NO_LEAN_TILES: interior tiles of the fused sweep take the general body too
    long long no_staged_coef = 0;         // SOMAR_NO_STAGED_COEF: the streamed fused sweep loads its coefficients into registers in the step that uses them
    long long staged_min_cells = 4194304; // SOMAR_STAGED_MIN_CELLS: ... on levels smaller than this too: the staging through LDS did not pay at 128^3 (tests: 0)
    // ---- metric flags (PressureSolver::detect_metric_flags) ----
    long long no_uniform = 0;             // SOMAR_NO_UNIFORM: stream constant coefficient arrays anyway
    long long no_zero_planes = 0;         // SOMAR_NO_ZERO_PLANES: multiply identically zero J g^{xy} planes anyway
    // ---- V-cycle folding steps ----
    long long no_zero_start = 0;          // SOMAR_NO_ZERO_START: a zero correction comes from a memset, not from the sweep's in_mode 1
    long long no_fold_prolong = 0;        // SOMAR_NO_FOLD_PROLONG: prolongation / mean removal as passes of their own (also: no fp32 depths)
    long long no_cf_fused = 0;            // SOMAR_NO_CF_FUSED: levels with coarse-fine faces stay on the two-pass colour kernel
    long long amr_plain = 0;              // SOMAR_AMR_PLAIN: the plain AMR V-cycle instead of the lean one
    // ---- bottom solver ----
    long long fused_bottom_max_cells = 512;   // SOMAR_FUSED_BOTTOM_MAX_CELLS: k_tiny_bicgstab takes bottoms of at most this many cells (0: off)
    long long box_bottom = 1;             // SOMAR_BOX_BOTTOM: the persistent workgroup-per-box bottom solver (k_box_bicgstab), 0: off
    long long box_bottom_min_cells = 513; // SOMAR_BOX_BOTTOM_MIN_CELLS: smaller multi-box bottoms stay with k_tiny_bicgstab
    long long box_timing = 0;             // SOMAR_BOX_TIMING: k_box_bicgstab's phase timers
    long long bottom_async = 1;           // SOMAR_BOTTOM_ASYNC: graph_cycle reads the bottom's (iterations, exit) after enqueueing the up leg, 0: at once
    // ---- reductions and scalar fetches ----
    long long ordered_reduce_max = 4096;  // SOMAR_ORDERED_REDUCE_MAX: levels up to this many cells sum in the reference's serial order
    long long ordered_serial = 0;         // SOMAR_ORDERED_SERIAL: ... as one chain over all boxes instead of box-parallel chains
    long long no_fused_publish = 0;       // SOMAR_NO_FUSED_PUBLISH: a publish kernel of its own behind every reduction
    long long poll_fetch = 1;             // SOMAR_POLL_FETCH: the host spins on a published sequence number, 0: copy + synchronize
    // ---- non-diagonal metric, AMR ----
    long long ghost_staged = 0;           // SOMAR_GHOST_STAGED: ghost programs of small levels stage by stage, not as one launch
    long long no_ghost_dce = 0;           // SOMAR_NO_GHOST_DCE: no dead-op elimination in the ghost programs
    long long flux_fields = 0;            // SOMAR_FLUX_FIELDS: the flux register reads whole face fields
    long long fused19_min_box = -1;       // SOMAR_FUSED19_MIN_BOX: fused red+black 19-point sweep from this box width (negative: never; tests: 0)
    long long cf_full_gather = 0;         // SOMAR_CF_FULL_GATHER: coarse-fine interpolation gathers whole boxes, not their ghost ring
    // ---- exchange, graphs, ranks ----
    long long pull_max_cells = 262144;    // SOMAR_PULL_MAX_CELLS: single-rank levels up to this size refresh ghosts inside the stencil kernels
    long long graph_cells = 262144;       // SOMAR_GRAPH_CELLS: depths up to this size are replayed as HIP graphs (0: off)
    long long agglom_cells = 2097152;     // SOMAR_AGGLOM_CELLS: sharded depths up to this size are replicated on every rank
    long long no_overlap = 0;             // SOMAR_NO_OVERLAP: ghost messages on the compute stream, not under the interior tiles
    // ---- diagnostics ----
    long long timing = 0;                 // SOMAR_TIMING: 1: stage times of define / finalize / refresh on stderr, 2: + ghost program structure

    static Tuning from_env();
    // the value held for the switch SOMAR_<name>; false: no such switch
    bool get(const char* name, long long* value) const;
};

}  // namespace somar
