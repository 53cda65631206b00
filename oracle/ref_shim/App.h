// App.h — stand-in for the one declaration of the reference's App.h that its filter source needs.
//
// TEST INFRASTRUCTURE ONLY, written by this project.  The application class, its windowing and its scene types are not needed by the
// filter and are not restated.  cudaFramebuffer is, as in the reference's App.h:41-44, a struct of four texture-object handles in the order
// position, normal, UV, motion; the member names are the ones the filter source spells, the declaration is this project's own.
#pragma once

#include "ref_cuda_runtime.h"
#include <glm/glm.hpp>

namespace gpupt {
struct cudaFramebuffer {
    cudaTextureObject_t PositionTexture;      // unused by the filter
    cudaTextureObject_t NormalTexture;        // four 16-bit channels: half bits of the normal, material id
    cudaTextureObject_t UVTexture;            // four 16-bit channels: half bits of the barycentrics, instance id
    cudaTextureObject_t MotionTexture;        // four floats: motion x, y, depth, depth derivative
};
}  // namespace gpupt
