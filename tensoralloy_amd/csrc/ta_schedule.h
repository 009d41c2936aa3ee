// When the device MD loop samples: the schedule that every sampler of the loop keeps an instance of (MdSampler in
// ta_context.h; the sample_every of each is its own). Plain C++ with no HIP include (tests/test_schedule_cpu.py
// compiles it alone).
#pragma once
#include <algorithm>
#include <cstdint>

namespace ta {

// Samples are the whole-step states whose absolute step t (steps integrated since ta_md_init) is a multiple
// of `every` at or behind `origin`. Sample number and ring slot are functions of t alone, so a launch that is
// enqueued again after a list rebuild writes what it would have written.
struct SampleSchedule {
  int64_t every = 1;
  int64_t origin = 0;  // absolute step of sample 0 (a multiple of `every`)
  int64_t last = -1;   // absolute step of the newest sample, -1: none
  bool valid = false;  // the data are those of a run that succeeded

  // no sample held: sample 0 will be the first multiple of `every` at or behind the steps integrated so far
  void start(int64_t step_now) {
    origin = (step_now + every - 1) / every * every;
    last = -1;
  }
  // Launch k of a run that began at absolute step step0 holds the state t = step0 + k. Launch 0 does not
  // repeat the sample that the last launch of the run before took of that very state.
  bool due(int64_t step0, int64_t k) const {
    const int64_t t = step0 + k;
    return t >= origin && (t - origin) % every == 0 && !(k == 0 && t == last);
  }
  int64_t index(int64_t t) const { return (t - origin) / every; }  // sample number of step t
  int64_t step(int64_t n) const { return origin + n * every; }      // absolute step of sample n
  int64_t taken() const { return last < 0 ? 0 : index(last) + 1; }
  // after a run that ended at step_end: the newest sample is the last multiple of `every` reached
  void finish(int64_t step_end) {
    if (step_end >= origin) last = std::max(last, step(index(step_end)));
  }
  // a run begins: the data are invalid until it has succeeded, when the caller puts back what this returns
  bool suspend() {
    const bool was = valid;
    valid = false;
    return was;
  }
};

}  // namespace ta
