// train_mlp_wgrad_tpw1.hip -- tl_wgrad_kernel with one output tile per wave (train_mlp_wgrad_tpw.h). gfx950.
#include "train_mlp_wgrad_tpw.h"

namespace pn2 {
template int launch_wgrad_tpw<1>(const TlWgrad &p, const WgradShape &w, dim3 grid, hipStream_t st);
}
