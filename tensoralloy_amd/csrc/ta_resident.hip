// The host loop of the device-resident runs: what ta_md_run (ta_api_md.hip) and ta_relax_run
// (ta_api_relax.hip) share. Their launches are in ta_md.hip, ta_relax.hip and ta_neb.hip.
#include <cmath>
#include <cstring>

#include "ta_context.h"
#include "ta_md.h"

namespace ta {
namespace host {

void md_plan_blocks(ta_context *h, int chunk) {
  ResidentLoop &res = h->res;
  if (chunk == res.chunk && !res.blk_start_host.empty()) return;
  const size_t F = h->keep_natoms.size();
  std::vector<int32_t> &start = res.blk_start_host;
  start.assign(F + 1, 0);
  for (size_t f = 0; f < F; ++f)
    start[f + 1] = start[f] + std::max(1, (h->keep_natoms[f] + chunk - 1) / chunk);
  res.blk_start.ensure(F + 1);
  HIP_CHECK(hipStreamSynchronize(h->stream));  // (an earlier run's launches read the old layout)
  HIP_CHECK(hipMemcpy(res.blk_start.ptr, start.data(), (F + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
  res.chunk = chunk;
  res.n_blk = start[F];
}

void resident_begin(ta_context *h) {
  ResidentLoop &res = h->res;
  const size_t N = h->keep_species.size();
  if (res.ref_builds != h->n_list_builds) {  // the host built the list that is resident: its positions go up once
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (N) HIP_CHECK(hipMemcpy(res.ref.ptr, h->ref_pos.data(), 3 * N * sizeof(double), hipMemcpyHostToDevice));
    res.ref_builds = h->n_list_builds;
  }
  volatile unsigned *status_host = res.host_words();
  status_host[0] = status_host[1] = 0u;  // (no launch that writes them is in flight: every run ends with a wait)
  HIP_CHECK(hipMemsetAsync(res.status.ptr, 0, 2 * sizeof(unsigned), h->stream));
}

// `enqueue(q)` puts the launches of step q on the stream (they are predicated on the status word and test the
// skin / 2 rule after their drift); this loop follows each with the exact list of the step and an evaluation,
// looks at the page-locked status word every kMdLookahead steps, and where a drift left the list stale rebuilds
// it from the device's positions and goes on behind that step. After a look that found the list valid,
// `finished(k, k_end)` may name the step in [k, k_end) from which on the launches moved nothing (-1: none): the
// loop ends there. F of the state at entry must be resident. `*rebuilds` counts the lists built, `*n_rebuilds`
// (may be null) follows it so that a run that fails reports what it did.
int resident_steps(ta_context *h, const char *who, int n_steps, uint32_t want, const std::function<void(int)> &enqueue,
                   const std::function<int(int, int)> &finished, int *rebuilds, int32_t *n_rebuilds) {
  ResidentLoop &res = h->res;
  const size_t N = h->keep_species.size();
  hipStream_t s = h->stream;
  volatile unsigned *status_host = res.host_words();
  const int look = h->skin > 0.0 ? ta::kMdLookahead : 1;
  std::vector<double> x, cells;
  const size_t F = h->keep_natoms.size();
  int k = 0;
  while (k < n_steps) {
    // steps k .. k_end - 1 without a look at the device: integrator, exact list of the step, evaluation
    const int k_end = (int)std::min<int64_t>(n_steps, (int64_t)k + look);
    for (int q = k; q < k_end; ++q) {
      enqueue(q);
      if (h->filtered) apply_filter(h);
      compute_impl(h, want, false, nullptr);
    }
    wait_stream(s, h->opt);
    h->upload_pending = false;
    const unsigned mark = status_host[0];
    if (mark == 0u) {
      const int fin = finished(k, k_end);
      if (fin >= 0) {
        h->n_list_reuses += fin - k;
        return fin;
      }
      h->n_list_reuses += k_end - k;
      k = k_end;
      continue;
    }
    // the drift of step q left the list stale: the launches behind it did nothing, the evaluations
    // behind it ran on the stale list and are overwritten now
    const int q = (int)mark - 1;
    if (q < k || q >= k_end) throw std::runtime_error(std::string(who) + ": inconsistent status word");
    h->n_list_reuses += q - k;
    x.resize(3 * N);
    if (N) HIP_CHECK(hipMemcpy(x.data(), h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    if (res.cell_running) {  // the cells moved on the device: ref_cells are those of the stale list
      cells.resize(9 * F);
      if (F) HIP_CHECK(hipMemcpy(cells.data(), h->db.cells, 9 * F * sizeof(double), hipMemcpyDeviceToHost));
      if (h->md.baro.running) {  // a scale factor that was no finite number > 0 left NaNs in its frame's cell
        for (size_t f = 0; f < F; ++f) {
          bool ok = true;
          for (int c = 0; c < 9; ++c) ok = ok && std::isfinite(cells[9 * f + c]);
          if (!ok) {
            h->have_batch = false;  // (positions and cells of the frame are lost)
            h->md.valid = false;
            throw std::invalid_argument(std::string(who) + ": the barostat's scale factor of frame " + std::to_string(f) +
                                        " at step " + std::to_string(q + 1) + " is not a finite number > 0");
          }
        }
      }
    }
    status_host[0] = 0u;
    HIP_CHECK(hipMemsetAsync(res.status.ptr, 0, 2 * sizeof(unsigned), s));
    try {
      rebuild_list(h, x.data(), res.cell_running ? cells.data() : nullptr);
    } catch (const HipError &e) {
      throw HipError(std::string(who) + ": list rebuild after step " + std::to_string(q + 1) + " failed: " + e.what());
    } catch (const std::exception &e) {
      throw std::runtime_error(std::string(who) + ": list rebuild after step " + std::to_string(q + 1) +
                               " failed: " + e.what());
    }
    if (N) HIP_CHECK(hipMemcpyAsync(res.ref.ptr, h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (res.cell_running && F) {
      if (h->md.baro.running)  // the barostat keeps the scale since the build, not the list's cells
        HIP_CHECK(hipMemcpyAsync(h->md.baro.scale.ptr, h->md.baro.ones.data(), 3 * F * sizeof(double), hipMemcpyHostToDevice, s));
      else
        HIP_CHECK(hipMemcpyAsync(res.ref_cells.ptr, h->db.cells, 9 * F * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    res.ref_builds = h->n_list_builds;
    compute_impl(h, want, false, nullptr);
    ++*rebuilds;
    if (n_rebuilds) *n_rebuilds = *rebuilds;
    k = q + 1;
  }
  return n_steps;
}

// The cells moved under a list built for others: one list for the final state, so that ref_pos and ref_cells (the
// host's image of the resident geometry) are what ta_update_positions, ta_step, ta_md_run, ta_relax_run and a
// fixed-cell run take them for. The evaluation is repeated on it; results agree up to summation order.
void resident_final_cells(ta_context *h, const char *who, uint32_t want, int *rebuilds, int32_t *n_rebuilds) {
  const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
  hipStream_t s = h->stream;
  std::vector<double> cells(9 * F);
  HIP_CHECK(hipMemcpy(cells.data(), h->db.cells, 9 * F * sizeof(double), hipMemcpyDeviceToHost));
  if (std::memcmp(cells.data(), h->ref_cells.data(), 9 * F * sizeof(double)) == 0) return;
  std::vector<double> x(3 * N);
  if (N) HIP_CHECK(hipMemcpy(x.data(), h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
  try {
    rebuild_list(h, x.data(), cells.data());
  } catch (const HipError &e) {
    throw HipError(std::string(who) + ": list rebuild for the final cells failed: " + e.what());
  } catch (const std::exception &e) {
    throw std::runtime_error(std::string(who) + ": list rebuild for the final cells failed: " + e.what());
  }
  if (N) HIP_CHECK(hipMemcpyAsync(h->res.ref.ptr, h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToDevice, s));
  h->res.ref_builds = h->n_list_builds;
  compute_impl(h, want, false, nullptr);
  HIP_CHECK(hipStreamSynchronize(s));
  h->upload_pending = false;
  ++*rebuilds;
  if (n_rebuilds) *n_rebuilds = *rebuilds;
}

}  // namespace host
}  // namespace ta
