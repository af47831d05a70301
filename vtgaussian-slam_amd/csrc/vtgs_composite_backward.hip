// vtgs_composite_backward.hip -- the backward composites libvtgs.so ships: the lane = pixel instantiations of
// composite_backward_mx (vtgs_composite_backward.h) for the single render, the dual render, and the dual render whose second
// image passes a gradient through its first channel only (B1).
#include "vtgs_composite_backward.h"

namespace vtgs {

template __global__ decltype(composite_backward_mx<4, false, true>) composite_backward_mx<4, false, true>;
template __global__ decltype(composite_backward_mx<4, true, true>) composite_backward_mx<4, true, true>;
template __global__ decltype(composite_backward_mx<4, true, true, true>) composite_backward_mx<4, true, true, true>;

}  // namespace vtgs
