// train_mlp_wgrad_tpw2.hip -- tl_wgrad_kernel with 2 output tiles per wave (train_mlp_wgrad_tpw.h). gfx950.
#include "train_mlp_wgrad_tpw.h"

namespace pn2 {
template int launch_wgrad_tpw<2>(const TlWgrad &p, const WgradShape &w, dim3 grid, hipStream_t st);
}
