// generate_data -- low-resolution frames from a high-resolution image through the
// image model (reference: src/generate_data.cpp:83-127, same flag names).  The
// degradation runs on the GPU through the drop-in ImageModel; additive noise is
// drawn on the host with std::normal_distribution (the reference's cv::randn
// stream cannot be reproduced without OpenCV).
#include <cstdio>
#include <memory>
#include <random>
#include <string>

#include "apps/model_flags.h"
#include "image/image_io.h"
#include "image_model/image_model.h"
#include "image_model/photometric.h"

using namespace super_resolution;

int main(int argc, char** argv) {
  app::Flags flags(argc, argv,
      "generate_data --input_image=<ENVI config | .pgm | .ppm> --output_image_dir=<dir>\n"
      "  [--output_image_extension=<pgm|ppm|''(ENVI)>] [--save_as=<path>] [--motion_sequence_path=<file>]\n"
      "  [--blur_radius=0] [--blur_sigma=0] [--noise_sigma=0] [--noise_seed=1]\n"
      "  [--downsampling_scale=2] [--number_of_frames=4]\n"
      "  not a reference flag: [--affine_motion_path=<file>] (per-frame affine motion, 'a b tx c d ty' per line, HR pixels;\n"
      "                        an error together with --motion_sequence_path)\n"
      "                        [--flow_motion_path=<file>] (a dense displacement field per frame: raw little-endian float64,\n"
      "                        [frames][2][H][W] = the (ux, uy) planes in HR pixels at the input image's size; an error together\n"
      "                        with --motion_sequence_path or --affine_motion_path)\n"
      "                        [--flow_lattice_path=<file>] (the same motion on a control lattice: one text line `step lw lh\n"
      "                        frames`, then the raw little-endian float64 nodes [frames][2][lh][lw], node (i, j) at HR pixel\n"
      "                        (i step, j step), interpolated bilinearly; an error together with any other motion flag)\n"
      "                        [--blur_kernel_path=<file>] (a free-form blur kernel instead of the Gaussian of --blur_radius /\n"
      "                        --blur_sigma: text, the odd size ksize <= 7, then ksize * ksize taps in row-major order)\n"
      "                        [--blur_bank_path=<file>] (a blur kernel per frame, per channel or per both instead of one blur:\n"
      "                        text, `mode ksize entries` with mode 1 = per frame, 2 = per channel, 3 = per frame and channel\n"
      "                        ([frame][channel]), then entries * ksize * ksize taps; a per-frame bank holds one entry per\n"
      "                        motion of the sequence; an error together with --blur_kernel_path)\n"
      "                        [--photometric_path=<file>] (per-frame exposure, 'gain bias' per line, the bias in pixel units\n"
      "                        0..1: applied to the noise-free frame, the noise is added after)");
  const std::string input_image = flags.Str("input_image");
  const std::string output_dir = flags.Str("output_image_dir");
  std::string extension = flags.Str("output_image_extension");
  const std::string save_as = flags.Str("save_as");
  const app::ModelFlags model = app::ReadModelFlags(&flags, 0, 0.0);
  ImageModelParameters parameters = model.parameters;
  const std::string& flow_motion_path = model.flow_motion_path;
  const std::string photometric_path = flags.Str("photometric_path");  // not a reference flag
  parameters.noise_sigma = flags.Double("noise_sigma", 0.0);  // 0..255 units (additive_noise_module.cpp:25-26)
  parameters.noise_seed = static_cast<uint64_t>(flags.Int("noise_seed", 1));
  parameters.scale = flags.Int("downsampling_scale", 2);
  const int number_of_frames = flags.Int("number_of_frames", 4);
  flags.RejectUnknown();
  flags.Require("input_image");
  if (!parameters.blur_bank_path.empty() && !parameters.blur_kernel_path.empty()) return app::RefuseBoth("--blur_bank_path", "--blur_kernel_path");
  if (app::RefuseBothMotionFiles(model)) return 1;
  if (!flow_motion_path.empty() && (!parameters.affine_motion_sequence_path.empty() || !parameters.motion_sequence_path.empty()))
    return app::Refuse("--flow_motion_path excludes --motion_sequence_path and --affine_motion_path.");
  if (app::RefuseBothFlowFiles(model)) return 1;
  if (!model.flow_lattice_path.empty() && (!parameters.affine_motion_sequence_path.empty() || !parameters.motion_sequence_path.empty()))
    return app::Refuse("--flow_lattice_path excludes --motion_sequence_path and --affine_motion_path.");

  const ImageData image_data = util::LoadImage(input_image);
  if (!save_as.empty()) {  // copy / convert only (generate_data.cpp:94-98)
    util::SaveImage(image_data, save_as);
    return 0;
  }
  flags.Require("output_image_dir");
  // --photometric_path: gain and bias act on the noise-free frame, so the model runs without its noise module and the
  // noise (one module, the same stream of draws) is added last
  PhotometricSequence photometric;
  std::unique_ptr<AdditiveNoiseModule> noise_after;
  if (!photometric_path.empty()) {
    photometric.LoadSequenceFromFile(photometric_path);
    if (photometric.GetNumFrames() < number_of_frames)
      return app::Refuse("--photometric_path holds %d frames, --number_of_frames asks for %d.", photometric.GetNumFrames(), number_of_frames);
    if (parameters.noise_sigma > 0.0) noise_after.reset(new AdditiveNoiseModule(parameters.noise_sigma, parameters.noise_seed));
    parameters.noise_sigma = 0.0;
  }
  if (!flow_motion_path.empty()) {
    parameters.flow_motion_sequence.LoadSequenceFromFile(flow_motion_path, image_data.GetImageSize().width, image_data.GetImageSize().height);
    if (parameters.flow_motion_sequence.GetNumMotions() < number_of_frames)
      return app::Refuse("--flow_motion_path holds %d frames, --number_of_frames asks for %d.",
                         parameters.flow_motion_sequence.GetNumMotions(), number_of_frames);
  }
  if (!model.flow_lattice_path.empty()) {  // the forward model samples the interpolated field: the lattice, expanded
    FlowLatticeSequence lattice;
    lattice.LoadSequenceFromFile(model.flow_lattice_path);
    if (lattice.GetNumMotions() < number_of_frames)
      return app::Refuse("--flow_lattice_path holds %d frames, --number_of_frames asks for %d.", lattice.GetNumMotions(), number_of_frames);
    parameters.flow_motion_sequence = lattice.Expand(image_data.GetImageSize().width, image_data.GetImageSize().height);
  }
  const ImageModel image_model = ImageModel::CreateImageModel(parameters);
  if (!extension.empty() && extension[0] != '.') extension = "." + extension;
  for (int i = 0; i < number_of_frames; ++i) {
    ImageData frame = image_model.ApplyToImage(image_data, i);  // incl. the AdditiveNoiseModule, if any
    if (!photometric.Empty()) photometric.ApplyToImage(&frame, i);
    if (noise_after) noise_after->ApplyToImage(&frame, i);
    const std::string path = output_dir + "/low_res_" + std::to_string(i) + extension;
    util::SaveImage(frame, path);
    std::printf("Generated output image %s\n", path.c_str());
  }
  return 0;
}
