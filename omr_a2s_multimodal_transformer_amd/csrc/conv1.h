// First layer of the encoder (Cin = 1, conv1.hip), as called from the dense-3x3 C entry points of conv.hip, which have
// checked that the call is the plain stride-1 case.  OMR_ERR_UNSUPPORTED for output widths other than 16 / 32.
#pragma once
#include <hip/hip_runtime.h>

int omr_conv1_fwd(int dtype, const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int COUT, int relu, hipStream_t s);
int omr_conv1_wgrad(int dtype, const void* x, const void* dy, float* dw, float* db, int B, int H, int W, int COUT, hipStream_t s);
