// solve_path_bicycle.hip -- solve/plant/shift/constraint kernels of OdeModel<PathBicycle>: the path-frame kinematic bicycle with steering-rate limits (Trajectory Tracking/test2.py).
#include "kernels.h"

MPCX_INSTANTIATE(OdeModel<PathBicycle>, path_bicycle, "mpcx::OdeModel<mpcx::PathBicycle>")
