// The records of a skidpad planner that more than one translation unit reads: the planner's state in HBM (SkidState) and what a
// step reports about it (SkidInfo).  skidpad_kernel.h plans with them; skid_device_kernel.h re-creates single planners and hands a
// step's records to a caller on the GPU.
#pragma once

#include "fsdp_device.h"

namespace fsdp {

constexpr int SKID_HIST = 32;  // > SKID_GROUP_MAX

struct SkidState {
  int32_t has_original, relocalized, index_along_path;
  int32_t reloc_step;             // the step (since the reset) whose relocalization attempt latched the transform
  int32_t index_hist[SKID_HIST];  // index_along_path after step g at [g % SKID_HIST]
  double orig[4];          // pose latched at the first relocalization attempt
  double translation[2];
  double right_calc[2];
  double rotation;
  double prev[PATH_POINTS][4];  // previous_paths[-1] (map frame once relocalized)
};

struct SkidInfo {  // what RelocalizationInformation / the planner state expose (relocalization_information.py:12-35)
  int32_t relocalized, index_along_path;
  double translation[2];
  double rotation;
};

}  // namespace fsdp
