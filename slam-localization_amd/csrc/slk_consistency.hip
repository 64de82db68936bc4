// Translation unit of the consistency kernels (slk_consistency.hpp): slk_nees / slk_sample_states.
#define SLK_INST_UNIT 1
#define SLK_CONSISTENCY_UNIT 1
#include <hip/hip_runtime.h>
#include "../../include/slk.h"
#include "slk_kernels.hpp"
#include "slk_consistency.hpp"
