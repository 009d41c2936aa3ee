// Driver of tests/test_options_cpu.py: options_from_env (csrc/ta_options.cpp) over a fake environment made
// of the NAME=VALUE arguments; prints one "field value" line per field of ta::Options.
#include <cstdio>
#include <cstring>
#include <string>

#include "ta_options.h"

static int g_argc;
static char **g_argv;

static const char *fake_get(const char *name) {
  const size_t n = std::strlen(name);
  for (int k = 1; k < g_argc; ++k)
    if (std::strncmp(g_argv[k], name, n) == 0 && g_argv[k][n] == '=') return g_argv[k] + n + 1;
  return nullptr;
}

int main(int argc, char **argv) {
  g_argc = argc;
  g_argv = argv;
  const ta::Options o = ta::options_from_env(fake_get);
#define SHOW(field) std::printf(#field " %d\n", (int)o.field)
  SHOW(no_jobs); SHOW(full_records); SHOW(no_own_sums); SHOW(no_list_filter); SHOW(filter_rev_kernel);
  SHOW(force_v1); SHOW(no_eta_chain); SHOW(staged_copy_dma); SHOW(mlp_tile_kernel); SHOW(mlp_wave_kernel);
  SHOW(mlp_quad_kernel); SHOW(mlp_da_global); SHOW(eam_nn_generic);
  SHOW(host_nl); SHOW(nl_two_pass); SHOW(nl_copy_starts); SHOW(sync_blocking);
  SHOW(eam_nn_tables);
  SHOW(fwd_wpe); SHOW(bwd_wpe); SHOW(gather_w); SHOW(copy_wg_per_cu); SHOW(copy_mode);
  SHOW(debug_no_triples); SHOW(debug_skip); SHOW(stagger_fwd); SHOW(stagger_bwd);
#undef SHOW
  std::printf("phase_stamps_out %s\n", o.phase_stamps_out.c_str());
  return 0;
}
