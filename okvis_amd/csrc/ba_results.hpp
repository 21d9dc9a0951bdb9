// The packed results record of one window, laid out ONCE: pack_results_kernel (ba_solve.hpp) writes it on the device, and every
// host reader — okvis_ba_fetch_results, okvis_ba_fetch_imu_caches, stage_results, okvis_ba_finish's single-window staging
// (ba_capi.hip and its parts) and WindowStore::take_results (ba_store.hpp) — takes its offsets from here.  No HIP in here:
// store_capi.hip sees it through ba_store.hpp.
//
//   pose [n_pose][7] | speed/bias [n_sb][9] | landmarks [n_lm][4] | quality [n_lm] | IMU reference biases [n_imu][9] |
//   preintegration records [n_imu][OKVIS_BA_IMU_CACHE_DOUBLES]        (all doubles)
#pragma once
#include <cstddef>

#include "../../include/okvis_amd_ba.h"

namespace ba {

struct ResultsLayout {
  struct Part {
    size_t off, bytes;
  };
  Part pose, sb, lm, quality, sb_ref, caches;
  size_t total;
  constexpr ResultsLayout(int n_pose, int n_sb, int n_lm, int n_imu)
      : pose{0, 56 * (size_t)n_pose},
        sb{pose.off + pose.bytes, 72 * (size_t)n_sb},
        lm{sb.off + sb.bytes, 32 * (size_t)n_lm},
        quality{lm.off + lm.bytes, 8 * (size_t)n_lm},
        sb_ref{quality.off + quality.bytes, 72 * (size_t)(n_imu > 0 ? n_imu : 0)},
        caches{sb_ref.off + sb_ref.bytes, 8 * (size_t)OKVIS_BA_IMU_CACHE_DOUBLES * (size_t)(n_imu > 0 ? n_imu : 0)},
        total(caches.off + caches.bytes) {}
};

}  // namespace ba
