// Translation unit of the one-wave NEES record kernel of slk_step_n (slk_trajectory.hpp).
#define SLK_INST_UNIT 1
#define SLK_TRAJ_UNIT 1
#include <hip/hip_runtime.h>
#include "../../include/slk.h"
#include "slk_kernels.hpp"
#include "slk_trajectory.hpp"
