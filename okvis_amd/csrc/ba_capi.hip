// C-ABI of the MI355X sliding-window BA backend (include/okvis_amd_ba.h): host-side structure building
// (the index arrays that replace okvis::ceres::Map's pointer graph), the HBM arena, kernel launches and
// hipGraph capture of the iteration sequence.  There is NO CPU compute path in this file: every numeric
// entry point ends in a kernel launch and fails with OKVIS_BA_ERR_NO_DEVICE without a GPU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/okvis_amd_ba.h"
#include "ba_imu.hpp"
#include "ba_chol_tiles.hpp"
#include "ba_cov.hpp"
#include "ba_lmcov.hpp"
#include "ba_predcov.hpp"
#include "ba_linearize.hpp"
#include "ba_linearize2.hpp"
#include "ba_schur2.hpp"
#include "ba_marg.hpp"
#include "ba_marg_tiles.hpp"
#include "ba_schur.hpp"
#include "ba_solve.hpp"
#include "ba_store.hpp"

using namespace ba;

// One translation unit, in parts:
#include "capi_solver.inc"        // records: HostWin, Arena, okvis_ba_solver, DebugWord
#include "capi_index_build.inc"   // batch_layout, build_batch, build_window and its helpers (the index build)
#include "capi_launch.inc"        // LDS sizes, the launch plan (make_plan) and the launches, sub-batch fork / join
// below: life cycle and options; capi_queries.inc (state get / set, fetches, queries, download, measurement hooks) and capi_upload.inc
// (upload, check_window, patch); begin / iterate / finish with the timed and cost variants; then capi_standalone.inc,
// capi_marginalize.inc, capi_covariance.inc, capi_landmark_covariance.inc and capi_predicted_measurement.inc

// =====================================================================================================
extern "C" {

int okvis_ba_abi_version(void) { return OKVIS_BA_ABI_VERSION; }

void okvis_ba_get_limits(okvis_ba_limits* out) {
  if (!out) return;
  out->max_obs_per_lm = GROUP_OBS;
  out->max_reduced_dim = MAX_D;
  out->max_marg_dim = MAX_MARG_DIM;
  out->max_imu_samples_per_factor = MAX_IMU_SAMPLES;
}

void okvis_ba_default_options(okvis_ba_options* o) {
  if (!o) return;
  // Ceres 1.9 defaults restated from its documentation (not in the reference tree)
  o->initial_radius = 1e4;
  o->max_radius = 1e16;
  o->min_radius = 1e-32;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->min_relative_decrease = 1e-3;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->use_graph = 1;
  o->schur_lm_per_block = 0;
  o->debug_arrays = 0;
  o->gauss_newton = 0;
  o->n_streams = 0;
  o->fp32_linearize = 0;
  o->strategy = OKVIS_BA_STRATEGY_DOGLEG;   // what the reference configures (Estimator.cpp:858)
  o->jacobi_scaling = 1;
  o->max_consecutive_invalid_steps = 5;
  o->reserved0 = 0;
  std::memset(&o->tuning, 0, sizeof(o->tuning));
}

const char* okvis_ba_error_string(int status) {
  switch (status) {
    case OKVIS_BA_OK: return "ok";
    case OKVIS_BA_ERR_ARG: return "invalid argument (null pointer, index out of range, unsorted/duplicate observations)";
    case OKVIS_BA_ERR_STATE: return "call order violated";
    case OKVIS_BA_ERR_UNSUPPORTED: return "structure exceeds a documented limit (okvis_ba_get_limits)";
    case OKVIS_BA_ERR_NO_DEVICE: return "no HIP device visible: this backend has no CPU path";
    case OKVIS_BA_ERR_NUMERIC: return "numeric failure";
  }
  if (status >= OKVIS_BA_HIP_ERROR_BASE) return hipGetErrorString((hipError_t)(status - OKVIS_BA_HIP_ERROR_BASE));
  return "unknown status";
}

int okvis_ba_create(okvis_ba_solver** out, int device) {
  if (!out) return OKVIS_BA_ERR_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return OKVIS_BA_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return OKVIS_BA_ERR_ARG;
  okvis_ba_solver* s = new okvis_ba_solver();
  s->device = device;
  okvis_ba_default_options(&s->opt);
  s->stagger_ticks = 10 * 100;   // start offset of the sub-batch streams (us; okvis_ba_tuning::stagger_us; round 2: 20 / 45 / 70 us all lock the fast interleaving; round 6: 5 and 10 us do too)
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&s->ev0);
  if (e == hipSuccess) e = hipEventCreate(&s->ev1);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming);
  // the word the three-launch iteration's solve kernel bumps when it pauses a window: page-locked, mapped, coherent
  if (e == hipSuccess) e = hipHostMalloc((void**)&s->h_pause, 64, hipHostMallocMapped | hipHostMallocCoherent);
  if (e == hipSuccess) {
    s->h_pause[0] = 0;
    e = hipHostGetDevicePointer((void**)&s->d_pause, s->h_pause, 0);
  }
  // the option record and the window records share one allocation — [OptD, padded | WinPtrs x capacity] — so that an upload
  // refreshes both with ONE copy
  if (e == hipSuccess) e = hipMalloc(&s->d_opt, records_bytes(1));
  if (e == hipSuccess) {
    s->d_wins = reinterpret_cast<WinPtrs*>(reinterpret_cast<unsigned char*>(s->d_opt) + OPT_PAD);
    s->d_ctrl = reinterpret_cast<CtrlSlot*>(reinterpret_cast<unsigned char*>(s->d_opt) + ctrl_off(1));
    s->wins_capacity = 1;
  }
  // kernels may use more than the default 64 KB of dynamic LDS
  auto lds = [&](auto f, size_t bytes) {
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(f), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  };
  for (const auto& k : plan_kernels()) lds(k.first, k.second);
  lds(&chol_tiles_window_kernel, CT_SMEM_DOUBLES * 8);
  lds(&marg_dense_kernel<MAX_D_LDS, MARG_SMALL_PRIOR>, MARG_LDS_DOUBLES * 8);
  lds(&marg_dense_kernel<MAX_D, MAX_MARG_DIM>, MARG_LDS_DOUBLES_LARGE * 8);
  lds(&cov_kernel, cov_lds_bytes(MAX_D_LDS));

  if (e != hipSuccess) {
    int code = OKVIS_BA_HIP_ERROR_BASE + (int)e;
    okvis_ba_destroy(s);
    return code;
  }
  *out = s;
  return OKVIS_BA_OK;
}

int okvis_ba_destroy(okvis_ba_solver* s) {
  if (!s) return OKVIS_BA_OK;
  (void)hipSetDevice(s->device);
  destroy_graphs(s);
  if (s->d_arena) (void)hipFree(s->d_arena);
  if (s->d_pre) (void)hipFree(s->d_pre);
  if (s->ev_marg_vals) (void)hipEventDestroy(s->ev_marg_vals);
  if (s->d_opt) (void)hipFree(s->d_opt);   // (d_wins lives in the same allocation)
  if (s->h_ctrl_stage) (void)hipHostFree(s->h_ctrl_stage);
  if (s->d_ctrl_stage) (void)hipFree(s->d_ctrl_stage);
  if (s->h_pause) (void)hipHostFree(s->h_pause);
  if (s->d_redo_mark) (void)hipFree(s->d_redo_mark);
  if (s->marg_scratch) (void)hipFree(s->marg_scratch);
  for (CovEvents* ev : {&s->ev_cov, &s->ev_lmcov, &s->ev_pred}) cov_events_destroy(*ev);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
  for (auto st : s->sub_streams)
    if (st != s->stream) (void)hipStreamDestroy(st);
  for (auto ev : s->sub_events) (void)hipEventDestroy(ev);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
  return OKVIS_BA_OK;
}

int okvis_ba_set_options(okvis_ba_solver* s, const okvis_ba_options* opt) {
  if (!s || !opt) return OKVIS_BA_ERR_ARG;
  if (!(opt->initial_radius > 0) || !(opt->min_lm_diagonal > 0) || !(opt->max_lm_diagonal >= opt->min_lm_diagonal))
    return OKVIS_BA_ERR_ARG;
  if (s->host.uploaded && (opt->debug_arrays != s->opt.debug_arrays || opt->schur_lm_per_block != s->opt.schur_lm_per_block ||
                      opt->n_streams != s->opt.n_streams))
    return OKVIS_BA_ERR_STATE;  // these shape the arena: set them before upload
  if (s->host.uploaded) {   // ... and so does the tuning record, but for the switches that are read per call and the stream stagger
    const uint32_t per_call = OKVIS_BA_TUNE_NO_MARG_TILES | OKVIS_BA_TUNE_NO_EARLY_PREINTEGRATION | OKVIS_BA_TUNE_H0_ON_HOST;
    okvis_ba_tuning a = opt->tuning, b = s->opt.tuning;
    a.flags &= ~per_call; b.flags &= ~per_call;
    a.stagger_us = b.stagger_us = 0;
    if (std::memcmp(&a, &b, sizeof(a)) != 0) return OKVIS_BA_ERR_STATE;
  }
  // unchanged options (the host class sets them before every upload): nothing to do - every upload writes the device copy
  if (std::memcmp(opt, &s->opt, sizeof(*opt)) == 0) return OKVIS_BA_OK;
  s->opt = *opt;
  if (s->host.uploaded) {   // the launches of the new options (captured graphs hold those of the old ones)
    s->plan = make_plan(s->layout, s->max, s->opt, (int)s->wins.size());
    keep_graphs(s);
  }
  s->stagger_ticks = (long long)(opt->tuning.stagger_us > 0 ? opt->tuning.stagger_us : opt->tuning.stagger_us < 0 ? 0 : 10) * 100;   // (round 6: 5 / 10 us 479 k, 20 us 476 k, 30 us 474 k, none 465 k at 64 windows)
  HIP_TRY(hipSetDevice(s->device));
  OptD d = make_optd(s->opt, (int)s->wins.size());
  HIP_TRY(hipMemcpyAsync(s->d_opt, &d, sizeof(d), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return OKVIS_BA_OK;
}

int okvis_ba_set_patchable(okvis_ba_solver* s, int on) {
  if (!s) return OKVIS_BA_ERR_ARG;
  s->patchable = on != 0;
  if (!s->patchable) s->mirrors.clear();
  return OKVIS_BA_OK;
}

#include "capi_queries.inc"       // state get / set, stage_results and the fetches, queries, okvis_ba_download, measurement hooks
#include "capi_upload.inc"        // pre_launch, upload_impl, okvis_ba_upload, okvis_ba_check_window[_lists], patch_window, marg prior values, patched_view

int okvis_ba_begin(okvis_ba_solver* s) {
  REFUSE_BETWEEN_MARG_HALVES(s);
  if (s) s->host.begin_entered();   // (before the checks: an okvis_ba_begin that is refused has still dropped what was staged)
  if (int rc = enter(s, ENTER_UPLOADED | ENTER_DEVICE)) return rc;
  s->host.slots_restart();
  {
    const size_t n = s->wins.size();
    HIP_TRY(reserve_ctrl_stage(s, n));
    int* accs = reinterpret_cast<int*>(s->h_ctrl_stage);
    for (size_t i = 0; i < n; ++i) accs[i] = s->wins[i].acc;
    HIP_TRY(hipMemcpyAsync(s->d_ctrl_stage, accs, sizeof(int) * n, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(begin_kernel, dim3((unsigned)n), dim3(256), 0, s->stream, s->d_wins, reinterpret_cast<const int*>(s->d_ctrl_stage),
                       s->opt.initial_radius);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(launch_lin(s, whole(s), 1));
  if (s->plan.three) {
    // the three-launch iteration: what the iterations re-preintegrate is counted from here (okvis_ba_finish reads it: start_four)
    const size_t n = s->wins.size();
    if (s->redo_mark_windows < n) {
      if (s->d_redo_mark) HIP_TRY(hipFree(s->d_redo_mark));
      s->d_redo_mark = nullptr, s->redo_mark_windows = 0;
      HIP_TRY(hipMalloc((void**)&s->d_redo_mark, sizeof(int) * n));
      s->redo_mark_windows = n;
    }
    hipLaunchKernelGGL(redo_mark_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s->stream, s->d_wins, s->d_redo_mark, (int)n);
    HIP_TRY(hipGetLastError());
  }
  // (pauses belong to one begin ... finish: whoever pauses a window resumes it before okvis_ba_finish returns)
  s->pause_begin = s->pause_seen = __atomic_load_n(s->h_pause, __ATOMIC_ACQUIRE);
  s->three_unseen = false;
  s->host.begin_done();
  return OKVIS_BA_OK;
}

// The route of the next iterations (true = four launches) and the host's part of the three-launch iteration: a three-launch call of
// this begin ... finish that nobody has waited for may have paused windows — they would sit out the whole next call — so it is
// waited for, and the word the pausing workgroups bump is looked at.  Unchanged: three launches.  Changed: the paused windows are
// brought level on the four-launch route (resume_paused) and the call that follows takes that route too — where one term moved past
// the threshold, others are about to.
static int settle_pauses(okvis_ba_solver* s, bool* four) {
  *four = true;
  if (!s->plan.three) return OKVIS_BA_OK;
  if (s->three_unseen) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->three_unseen = false;
  }
  const int word = __atomic_load_n(s->h_pause, __ATOMIC_ACQUIRE);
  if (word != s->pause_seen) {
    s->pause_seen = word;
    std::vector<Ctrl> cs;
    if (int rc = fetch_ctrl(s, cs)) return rc;
    int n_paused = 0;
    return resume_paused(s, cs, &n_paused);
  }
  *four = s->start_four;
  return OKVIS_BA_OK;
}

int okvis_ba_iterate(okvis_ba_solver* s, int n) {
  REFUSE_BETWEEN_MARG_HALVES(s);
  if (s) s->host.work_enqueued();
  if (int rc = enter(s, ENTER_BEGUN, 0, n >= 0)) return rc;
  if (n == 0) return OKVIS_BA_OK;
  s->host.iterations_enqueued();
  HIP_TRY(hipSetDevice(s->device));
  bool four = true;
  if (int rc = settle_pauses(s, &four)) return rc;
  if (s->plan.three && !four) s->three_unseen = true;
  s->host.slots_add(n);
  const int nsub = (int)s->sub_streams.size();
  // The graph of sub-batch k's chain (nsub > 1: one graph per sub-batch, each replayed on its own stream — independent launches
  // overlap; branches inside ONE captured graph were measured not to) or of the whole call (k = -1), on the route `r`: captured at
  // its first use.  A plan with the three-launch iteration captures a call length's graphs of BOTH routes at its first use: which
  // route a later call of that length takes is the device's news, and a caller who replays a call length it has issued before
  // expects no capture in it.
  auto graph_of = [&](int k, bool r, hipGraphExec_t* exec) -> int {
    const int key = graph_key(n, r);
    if (k >= 0) {
      auto it = s->sub_graphs.find({key, k});
      if (it != s->sub_graphs.end()) return *exec = it->second, OKVIS_BA_OK;
    } else {
      auto it = s->graphs.find(key);
      if (it != s->graphs.end()) return *exec = it->second, OKVIS_BA_OK;
    }
    hipGraph_t graph = nullptr;
    const hipStream_t st = k >= 0 ? s->sub_streams[k] : s->stream;
    HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    hipError_t e = k >= 0 ? launch_chain(s, sub(st, s->plan.subs[k]), n, n, r) : launch_iterations_forked(s, n, -1, r);
    hipError_t e2 = hipStreamEndCapture(st, &graph);
    if (e != hipSuccess) HIP_TRY(e);
    HIP_TRY(e2);
    HIP_TRY(hipGraphInstantiate(exec, graph, nullptr, nullptr, 0));
    HIP_TRY(hipGraphDestroy(graph));
    if (k >= 0) s->sub_graphs[{key, k}] = *exec;
    else s->graphs[key] = *exec;
    return OKVIS_BA_OK;
  };
  std::vector<hipGraphExec_t> execs;
  if (s->plan.graph) {
    for (int k = nsub > 1 ? 0 : -1; k < (nsub > 1 ? nsub : 0); ++k) {
      hipGraphExec_t exec = nullptr, other = nullptr;
      if (int rc = graph_of(k, four, &exec)) return rc;
      if (s->plan.three)
        if (int rc = graph_of(k, !four, &other)) return rc;
      execs.push_back(exec);
    }
  }
  HIP_TRY(hipEventRecord(s->ev0, s->stream));   // (behind the captures: a capture swallows an event record)
  if (s->plan.graph && nsub > 1) {
    HIP_TRY(hipEventRecord(s->ev_fork, s->stream));
    for (int k = 0; k < nsub; ++k) {
      HIP_TRY(hipStreamWaitEvent(s->sub_streams[k], s->ev_fork, 0));
      // the sub-batches start staggered by a third (1 / nsub) of one iteration chain: started together, the streams lock into
      // one of two interleavings (0.162 or 0.179 ms per step at 64 windows, whole timed regions in either); the stagger
      // starts them in the pipelined pattern
      if (k > 0 && s->stagger_ticks > 0) {
        hipLaunchKernelGGL(delay_kernel, dim3(1), dim3(64), 0, s->sub_streams[k], (long long)k * s->stagger_ticks);
        HIP_TRY(hipGetLastError());
      }
      HIP_TRY(hipGraphLaunch(execs[k], s->sub_streams[k]));
      HIP_TRY(hipEventRecord(s->sub_events[k], s->sub_streams[k]));
      HIP_TRY(hipStreamWaitEvent(s->stream, s->sub_events[k], 0));
    }
  } else if (s->plan.graph) {
    HIP_TRY(hipGraphLaunch(execs[0], s->stream));
  } else {
    HIP_TRY(launch_iterations_forked(s, n, -1, four));
  }
  HIP_TRY(hipEventRecord(s->ev1, s->stream));
  return OKVIS_BA_OK;
}

int okvis_ba_finish(okvis_ba_solver* s, okvis_ba_summary* summaries) {
  if (int rc = enter(s, ENTER_MARG_FIRST | ENTER_BEGUN | ENTER_DEVICE)) return rc;
  // landmark quality, the packed results of a one-window solver (the estimator's case: okvis_ba_fetch_results then costs no
  // launch, no copy and no synchronisation of its own) and the control records, all behind ONE synchronisation
  std::vector<Ctrl> cs;
  size_t res_bytes = 0;
  auto finalize = [&]() -> int {
    HIP_TRY(launch_imu_take_back(s, 0, (int)s->wins.size()));
    if (s->max.lm > 0) {
      hipLaunchKernelGGL(quality_kernel, dim3((s->max.lm + 255) / 256, (unsigned)s->wins.size()), dim3(256), 0, s->stream, s->d_wins);
      HIP_TRY(hipGetLastError());
    }
    if (s->wins.size() == 1) {
      const HostWin& H0 = s->wins[0];
      res_bytes = ResultsLayout(H0.n_pose, H0.n_sb, H0.n_lm, H0.n_imu).total;
      if (res_bytes) {
        s->stage_res.resize(res_bytes);
        hipLaunchKernelGGL(pack_results_kernel, dim3(8), dim3(256), 0, s->stream, s->d_wins, -1);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(s->stage_res.data(), H0.ptrs.results, res_bytes, hipMemcpyDeviceToHost, s->stream));
      }
    }
    return fetch_ctrl(s, cs, s->plan.three != 0);
  };
  // the final accept/reject needs the Schur partials of the buffer it may accept (gradient test); then what hangs on it
  auto decide = [&]() -> int {
    HIP_TRY(launch_schur(s, whole(s), 1));
    HIP_TRY(launch_solve(s, whole(s), 1));
    return finalize();
  };
  int rc = decide();
  if (rc != OKVIS_BA_OK) return rc;
  if (s->plan.three) {
    // The three-launch iteration: a window the solve kernel paused (the launches above skipped it like a finished one) still owes
    // iterations.  It gets them on the four-launch route, where nothing pauses; then the final decision is taken again.
    s->three_unseen = false;
    int n_paused = 0;
    if ((rc = resume_paused(s, cs, &n_paused)) != OKVIS_BA_OK) return rc;
    if (n_paused > 0 && (rc = decide()) != OKVIS_BA_OK) return rc;
    // the next begin ... finish starts on the four-launch route if this one paused or re-preintegrated: its windows are on the move
    long redone = 0;
    for (const Ctrl& c : cs) redone += c.pad2;
    s->pause_seen = __atomic_load_n(s->h_pause, __ATOMIC_ACQUIRE);
    s->start_four = s->pause_seen != s->pause_begin || redone > 0;
  }
  if (s->opt.strategy == OKVIS_BA_STRATEGY_DOGLEG && !s->opt.gauss_newton) {
    // Dogleg: a launch slot that had to redo a mis-speculated Gauss-Newton trial as an explicit dogleg step did not
    // finish an iteration, and the decision just taken may itself ask for such a redo.  Windows that still owe
    // iterations of this call's budget get the missing slots (the others are stopped by the budget), then the final
    // decision (and what hangs on it) is taken again.  Rare: only when the Gauss-Newton point lies outside the trust region —
    // the common case pays one synchronisation for the whole finish.
    for (int round = 0; round < 64 && !s->skip_topup; ++round) {
      int need = 0;
      for (const Ctrl& c : cs) {
        if (c.done) continue;
        int k = c.max_iter - c.iter;
        if (c.explicit_next == 2) k += 1;   // the current iteration itself is unfinished
        need = std::max(need, k);
      }
      if (need <= 0) break;
      s->host.slots_add(need);
      HIP_TRY(launch_iterations_forked(s, need, 0, true));   // (on the sub-batch streams like every other iteration; no new budget)
      if ((rc = decide()) != OKVIS_BA_OK) return rc;
    }
  }
  for (size_t i = 0; i < s->wins.size(); ++i) {
    s->wins[i].acc = cs[i].acc;
    if (summaries) {
      okvis_ba_summary& o = summaries[i];
      o.initial_cost = cs[i].initial_cost;
      o.final_cost = cs[i].cost;
      o.iterations = cs[i].iter;
      o.successful_steps = cs[i].successful;
      o.termination = cs[i].done ? (cs[i].done - 1 == 6 ? 0 : cs[i].done - 1) : 0;   // 6 = budget used up = max iterations
      o.reserved = cs[i].chol_fail;
      o.final_radius = cs[i].radius;
      o.gradient_max_norm = cs[i].grad_max;
    }
  }
  s->host.finish_done(res_bytes > 0);
  return OKVIS_BA_OK;
}

int okvis_ba_optimize(okvis_ba_solver* s, int num_iter, okvis_ba_summary* summaries) {
  int rc = okvis_ba_begin(s);
  if (rc != OKVIS_BA_OK) return rc;
  rc = okvis_ba_iterate(s, num_iter);
  if (rc != OKVIS_BA_OK) return rc;
  return okvis_ba_finish(s, summaries);
}

int okvis_ba_optimize_timed(okvis_ba_solver* s, int max_iter, int min_iter, double time_limit_s,
                            okvis_ba_summary* summaries) {
  if (!s || max_iter < 0 || min_iter < 0) return OKVIS_BA_ERR_ARG;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = okvis_ba_begin(s);
  if (rc != OKVIS_BA_OK) return rc;
  int done = 0;
  if (time_limit_s < 0) {  // Estimator::setOptimizationTimeLimit: no limit -> min iterations = max iterations
    rc = okvis_ba_iterate(s, max_iter);
    if (rc != OKVIS_BA_OK) return rc;
  } else {
    const int first = std::min(min_iter, max_iter);
    rc = okvis_ba_iterate(s, first);
    if (rc != OKVIS_BA_OK) return rc;
    done = first;
    // CeresIterationCallback.hpp:77-86: stop once iteration >= min and the time budget is exceeded
    while (done < max_iter) {
      HIP_TRY(hipStreamSynchronize(s->stream));
      const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (done >= min_iter && el > time_limit_s) {
        s->skip_topup = true;   // the time limit ends the call (CeresIterationCallback terminates the solve)
        break;
      }
      rc = okvis_ba_iterate(s, 1);
      if (rc != OKVIS_BA_OK) return rc;
      ++done;
    }
  }
  rc = okvis_ba_finish(s, summaries);
  s->skip_topup = false;
  return rc;
}

int okvis_ba_evaluate_cost(okvis_ba_solver* s, double* costs) {
  if (s) s->host.work_enqueued();
  if (!s || !costs) return OKVIS_BA_ERR_ARG;
  int rc = okvis_ba_begin(s);
  if (rc != OKVIS_BA_OK) return rc;
  std::vector<okvis_ba_summary> sum(s->wins.size());
  rc = okvis_ba_finish(s, sum.data());
  if (rc != OKVIS_BA_OK) return rc;
  for (size_t i = 0; i < sum.size(); ++i) costs[i] = sum[i].final_cost;
  return OKVIS_BA_OK;
}

int okvis_ba_synchronize(okvis_ba_solver* s) {
  if (int rc = enter(s, ENTER_DEVICE)) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return OKVIS_BA_OK;
}

#include "capi_standalone.inc"    // okvis_ba_shard, okvis_ba_batch_run, okvis_ba_dense_solve, okvis_ba_reduced_solve

#include "capi_marginalize.inc"   // okvis_ba_marginalize, _begin, _end; okvis_ba_marginalize_batch, _batch_begin, _batch_end

#include "capi_covariance.inc"    // okvis_ba_state_covariance
#include "capi_landmark_covariance.inc"   // okvis_ba_landmark_covariance
#include "capi_predicted_measurement.inc"   // okvis_ba_predicted_measurement

}  // extern "C"
