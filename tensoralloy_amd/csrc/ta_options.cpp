// The one place where the library reads its environment (see ta_options.h).
#include "ta_options.h"

#include <cstdio>
#include <cstdlib>

namespace ta {

namespace {

// "<count>[,<shift>]" -> bits 8-15 and 16-20 of a launch's flag word
int stagger_flag(const char *e) {
  int n = 0, shift = 3;
  if (!e || std::sscanf(e, "%d,%d", &n, &shift) < 1) return 0;
  return ((n & 0xff) << 8) | ((shift & 31) << 16);
}

}  // namespace

Options options_from_env(const char *(*get)(const char *)) {
  Options o;
  const auto set = [&](const char *name) { return get(name) != nullptr; };
  const auto first_is = [&](const char *name, char c) {
    const char *v = get(name);
    return v && v[0] == c;
  };
  const auto number = [&](const char *name, int unset) {
    const char *v = get(name);
    return v ? std::atoi(v) : unset;
  };
  o.no_jobs = set("TA_NO_JOBS");
  o.full_records = set("TA_FULL_RECORDS");
  o.no_own_sums = set("TA_NO_OWN_SUMS");
  o.no_list_filter = set("TA_NO_LIST_FILTER");
  o.filter_rev_kernel = set("TA_FILTER_REV_KERNEL");
  o.force_v1 = set("TA_FORCE_V1");
  o.no_eta_chain = set("TA_NO_ETA_CHAIN");
  o.staged_copy_dma = set("TA_STAGED_COPY_DMA");
  o.mlp_tile_kernel = set("TA_MLP_TILE_KERNEL");
  o.mlp_wave_kernel = set("TA_MLP_WAVE_KERNEL");
  o.mlp_quad_kernel = set("TA_MLP_QUAD_KERNEL");
  o.mlp_da_global = set("TA_MLP_DA_GLOBAL");
  o.eam_nn_generic = set("TA_EAM_NN_GENERIC");
  o.host_nl = first_is("TA_HOST_NL", '1');
  o.nl_two_pass = first_is("TA_NL_TWO_PASS", '1');
  o.nl_copy_starts = first_is("TA_NL_COPY_STARTS", '1');
  o.sync_blocking = first_is("TA_SYNC_BLOCKING", '1');
  o.mlp_tile_generic = first_is("TA_MLP_TILE_GENERIC", '1');
  o.eam_nn_tables = !first_is("TA_EAM_NN_TABLES", '0');
  o.fwd_wpe = number("TA_FWD_WPE", 0);
  o.bwd_wpe = number("TA_BWD_WPE", 0);
  o.gather_w = number("TA_GATHER_W", 0);
  o.copy_wg_per_cu = number("TA_COPY_WG_PER_CU", 8);
  o.copy_mode = number("TA_COPY_MODE", -1);
  if (const char *v = get("TA_PHASE_STAMPS_OUT")) o.phase_stamps_out = v;
  o.debug_no_triples = set("TA_DEBUG_NO_TRIPLES");
  if (const char *v = get("TA_DEBUG_SKIP")) o.debug_skip = std::atoi(v) & 127;
  o.stagger_fwd = stagger_flag(get("TA_STAGGER_FWD"));
  o.stagger_bwd = stagger_flag(get("TA_STAGGER_BWD"));
  return o;
}

Options options_from_env() {
  return options_from_env([](const char *name) -> const char * { return std::getenv(name); });
}

}  // namespace ta
