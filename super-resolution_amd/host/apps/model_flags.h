// The image-model flags that generate_data and super_resolution both read, and the exclusion both state in the same words.
#pragma once
#include <string>

#include "apps/app_flags.h"
#include "image_model/image_model.h"
#include "motion/flow_lattice.h"

namespace super_resolution {
namespace app {

struct ModelFlags {
  ImageModelParameters parameters;  // the two sequence paths, the blur flags; the tool fills in its scale and noise
  std::string flow_motion_path;     // the file has no header: the tool loads it once it knows the HR geometry
  std::string flow_lattice_path;    // the same motion on a control lattice (motion/flow_lattice.h): expanded at the HR geometry
};

// --motion_sequence_path --affine_motion_path --flow_motion_path --flow_lattice_path --blur_radius --blur_sigma --blur_kernel_path --blur_bank_path;
// only the first and the Gaussian are reference flags, whose defaults differ between the tools
inline ModelFlags ReadModelFlags(Flags* flags, const int default_blur_radius, const double default_blur_sigma) {
  ModelFlags m;
  m.parameters.motion_sequence_path = flags->Str("motion_sequence_path");
  m.parameters.affine_motion_sequence_path = flags->Str("affine_motion_path");
  m.flow_motion_path = flags->Str("flow_motion_path");
  m.flow_lattice_path = flags->Str("flow_lattice_path");
  m.parameters.blur_radius = flags->Int("blur_radius", default_blur_radius);
  m.parameters.blur_sigma = flags->Double("blur_sigma", default_blur_sigma);
  m.parameters.blur_kernel_path = flags->Str("blur_kernel_path");
  m.parameters.blur_bank_path = flags->Str("blur_bank_path");
  return m;
}

// a model has one MotionModule: 1 after the refusal when both sequence files are given, else 0
inline int RefuseBothMotionFiles(const ModelFlags& m) {
  if (m.parameters.affine_motion_sequence_path.empty() || m.parameters.motion_sequence_path.empty()) return 0;
  return RefuseBoth("--affine_motion_path", "--motion_sequence_path");
}

// --flow_lattice_path gives the displacement field, as --flow_motion_path does: 1 after the refusal when both are given
inline int RefuseBothFlowFiles(const ModelFlags& m) {
  if (m.flow_motion_path.empty() || m.flow_lattice_path.empty()) return 0;
  return RefuseBoth("--flow_lattice_path", "--flow_motion_path");
}

}  // namespace app
}  // namespace super_resolution
