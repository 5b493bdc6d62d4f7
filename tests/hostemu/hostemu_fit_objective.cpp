// TEST-ONLY host build of the size of smplfit_fit_objective_f32's argument struct, compiled with g++ by
// tests/test_fitter_opt_host.py.
#include <cstddef>

#include "../../include/smplfit.h"

extern "C" {

int hostemu_sizeof_fit_objective_args() { return (int)sizeof(smplfit_fit_objective_args); }

}  // extern "C"
