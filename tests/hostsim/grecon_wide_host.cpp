// TEST INFRASTRUCTURE: the stage launcher's plan under the rules of the 32-person build -- grecon_launch.hpp seen the way csrc/grecon_wide.hip
// sees it.  Exports the plan only (stage_plan_shim.hpp); the algorithm itself is not instantiated.  Never loaded by the product.
#define GLAMR_GRECON_WIDE 1
#define GLAMR_MAX_PERSONS 32
#define GLAMR_GRECON_NS grecon_wide
#include "stage_plan_shim.hpp"
