// Translation unit of the ensemble kernels (slk_ensemble.hpp): slk_ensemble_moments / slk_gather_states.
#define SLK_INST_UNIT 1
#define SLK_ENSEMBLE_UNIT 1
#include <hip/hip_runtime.h>
#include "../../include/slk.h"
#include "slk_kernels.hpp"
#include "slk_ensemble.hpp"
