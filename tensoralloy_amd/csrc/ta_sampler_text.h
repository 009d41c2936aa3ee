// What the error messages say about each sampler of the device MD loop (ta_md_set_sampling, _rdf, _adf, _order,
// _clusters, _cna, _sq, _flux), and the functions that compose them. The texts are part of the documented behaviour.
// Plain C++ with no HIP include (tests/test_md_sampler_text_cpu.py compiles it alone).
#pragma once
#include <string>

namespace ta {

struct MdSamplerText {
  const char *setter;  // the entry point that switches the sampler on
  const char *off;     // what a getter says while it is off
  const char *data;    // what a failed ta_md_run leaves invalid
  const char *held;    // what ta_md_init finds no device memory for
  const char *gone;    // how a no-memory message ends
};

namespace md_text {
constexpr MdSamplerText corr = {"ta_md_set_sampling", "sampling is off", "sampled data", "rings", "sampling is off"};
constexpr MdSamplerText rdf = {"ta_md_set_rdf", "the pair distributions are off", "counts", "counts", "the feature is off"};
constexpr MdSamplerText adf = {"ta_md_set_adf", "the bond-angle distributions are off", "counts", "counts", "the feature is off"};
constexpr MdSamplerText order = {"ta_md_set_order", "the bond-orientational order parameters are off", "counts", "buffers",
                                 "the feature is off"};
constexpr MdSamplerText cluster = {"ta_md_set_clusters", "the cluster analysis is off", "data", "buffers", "the feature is off"};
constexpr MdSamplerText cna = {"ta_md_set_cna", "the common neighbour analysis is off", "data", "buffers", "the feature is off"};
constexpr MdSamplerText sq = {"ta_md_set_sq", "the structure factors are off", "data", "buffers", "the feature is off"};
constexpr MdSamplerText flux = {"ta_md_set_flux", "the heat current and pressure tensor are off", "data", "buffers",
                                "the feature is off"};
}  // namespace md_text

// `who` (a getter) found the sampler off
inline std::string md_text_off(const MdSamplerText &t, const std::string &who) {
  return who + ": " + t.off + " (" + t.setter + ")";
}
// `who` found the data of a run that failed
inline std::string md_text_invalid(const MdSamplerText &t, const std::string &who) {
  return who + ": a ta_md_run failed and left the " + t.data + " invalid; call " + t.setter + " or ta_md_init again";
}
// `who` (ta_md_init, or the setter with the sizes in `what`) found no device memory for `what`
inline std::string md_text_nomem(const MdSamplerText &t, const std::string &who, const std::string &what) {
  return who + ": no device memory for " + what + "; " + t.gone;
}
inline std::string md_text_init_nomem(const MdSamplerText &t) {
  return md_text_nomem(t, "ta_md_init", std::string("the ") + t.held + " of " + t.setter);
}

}  // namespace ta
