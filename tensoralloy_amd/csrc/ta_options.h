// The library's environment switches: read once per handle, in ta_create, and handed to the
// launchers and planners as arguments from there (DESIGN.md has the table). Pure host C++.
#pragma once
#include <string>

namespace ta {

struct Options {
  // set at all (any value, "0" included)
  bool no_jobs = false;            // TA_NO_JOBS: angular kernels without job lists (per-lane masks + re-dealing)
  bool full_records = false;       // TA_FULL_RECORDS: 64-byte pair records instead of the 32-byte {D, r^2}
  bool no_own_sums = false;        // TA_NO_OWN_SUMS: GRAP backward pass without the own-centre sums
  bool no_list_filter = false;     // TA_NO_LIST_FILTER: evaluate on the skin list itself
  bool filter_rev_kernel = false;  // TA_FILTER_REV_KERNEL: reverse-index launch behind the list filter
  bool force_v1 = false;           // TA_FORCE_V1: first-generation angular kernels
  bool no_eta_chain = false;       // TA_NO_ETA_CHAIN: every radial exponential evaluated on its own
  bool staged_copy_dma = false;    // TA_STAGED_COPY_DMA: small staged transfers through the DMA engine
  bool mlp_tile_kernel = false;    // TA_MLP_TILE_KERNEL: the generic tile kernel for every launch
  bool mlp_wave_kernel = false;    // TA_MLP_WAVE_KERNEL: the one-wavefront kernel below its tile threshold
  bool mlp_quad_kernel = false;    // TA_MLP_QUAD_KERNEL: the four / eight-wavefront kernel at every tile count
  bool mlp_da_global = false;      // TA_MLP_DA_GLOBAL: act' slab of the tile kernels in global memory
  bool eam_nn_generic = false;     // TA_EAM_NN_GENERIC: generic kernel for the nn pair functions
  // first character is '1'
  bool host_nl = false;         // TA_HOST_NL: neighbour lists by the host builder
  bool nl_two_pass = false;     // TA_NL_TWO_PASS: two-pass device builder only
  bool nl_copy_starts = false;  // TA_NL_COPY_STARTS: per-atom offsets by a copy, not written by the builder
  bool sync_blocking = false;   // TA_SYNC_BLOCKING: no polling before a blocking wait for the stream
  bool mlp_tile_generic = false;  // TA_MLP_TILE_GENERIC: the generic body of the tile kernels for every network
  // first character '0' switches off
  bool eam_nn_tables = true;  // TA_EAM_NN_TABLES: nn pair functions through their Hermite tables
  // atoi
  int fwd_wpe = 0;         // TA_FWD_WPE: 5 = the 96-register forward build
  int bwd_wpe = 0;         // TA_BWD_WPE: 4 / 6 = the 4- / 6-wavefront backward builds
  int gather_w = 0;        // TA_GATHER_W: 16 / 32 = lanes per atom of the force gather
  int copy_wg_per_cu = 8;  // TA_COPY_WG_PER_CU: grid of ta_measure_hbm_copy
  int copy_mode = -1;      // TA_COPY_MODE: >= 0 = the only copy method ta_measure_hbm_copy times
  // TA_PHASE_STAMPS_OUT: where a -DTA_PHASE_STAMPS build writes its stamps (empty: nowhere)
  std::string phase_stamps_out;
  // probe switches, consulted by -DTA_PROBE_SWITCHES builds only (wrong results by design)
  bool debug_no_triples = false;  // TA_DEBUG_NO_TRIPLES
  int debug_skip = -1;            // TA_DEBUG_SKIP: the low 7 bits of atoi, -1 = unset
  int stagger_fwd = 0;            // TA_STAGGER_FWD, TA_STAGGER_BWD: "<count>[,<shift>]" as the launch's flag
  int stagger_bwd = 0;            //   bits 8-20 (0: unset or unreadable)
};

// `get` returns a variable's value or null
Options options_from_env(const char *(*get)(const char *));
Options options_from_env();  // from the process environment

}  // namespace ta
