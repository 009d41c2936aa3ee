// Stand-alone driver of the samplers' message texts (csrc/ta_sampler_text.h) for tests/test_md_sampler_text_cpu.py.
// stdout, for each of the seven samplers in their canonical order, three lines: what the getter `ta_md_get_x` says
// while the sampler is off, what it says after a run that failed, and what ta_md_init says when it finds no device
// memory for the sampler.
#include <cstdio>

#include "ta_sampler_text.h"

int main() {
  const ta::MdSamplerText *all[] = {&ta::md_text::corr,    &ta::md_text::rdf, &ta::md_text::adf, &ta::md_text::order,
                                    &ta::md_text::cluster, &ta::md_text::cna, &ta::md_text::sq};
  for (const ta::MdSamplerText *t : all) {
    std::printf("%s\n", ta::md_text_off(*t, "ta_md_get_x").c_str());
    std::printf("%s\n", ta::md_text_invalid(*t, "ta_md_get_x").c_str());
    std::printf("%s\n", ta::md_text_init_nomem(*t).c_str());
  }
  return 0;
}
