// Stand-alone driver of ta::SampleSchedule (csrc/ta_schedule.h) for tests/test_schedule_cpu.py.
// stdin, one case per line:  every start n_runs len_1 .. len_n
// The schedule is started at absolute step `start`, then every run enqueues its launches k = 0 .. len (launch
// `len` finishes the last step, as ta_md_run's does) and finishes. stdout, per case: "C", then per run
//   S t i t i ...   the launches that were due: absolute step and sample index
//   R t i t i ...   every launch of the run asked again before the run ends (a replay after a list rebuild)
//   L last taken    the newest sample after the run and the samples taken so far
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <vector>

#include "ta_schedule.h"

int main() {
  long long every, start, n_runs;
  while (std::cin >> every >> start >> n_runs) {
    std::vector<long long> len(n_runs);
    for (auto &n : len) std::cin >> n;
    ta::SampleSchedule s;
    s.every = every;
    s.start(start);
    int64_t step = start;
    std::printf("C\n");
    for (long long n : len) {
      for (const char *tag : {"S", "R"}) {
        std::printf("%s", tag);
        for (long long k = 0; k <= n; ++k)
          if (s.due(step, k)) std::printf(" %lld %lld", (long long)(step + k), (long long)s.index(step + k));
        std::printf("\n");
      }
      step += n;
      s.finish(step);
      std::printf("L %lld %lld\n", (long long)s.last, (long long)s.taken());
    }
  }
  return 0;
}
