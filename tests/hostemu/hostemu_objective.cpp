// TEST-ONLY host build of the per-vertex arithmetic of smplfit_mesh_objective_f32 (sf::mesh_objective_vertex in
// csrc/sf_stages.h) and of the size of its argument struct, compiled with g++ by tests/test_flipper_opt_host.py.
#include <cstddef>

#include "../../include/smplfit.h"
#include "../../smplfitter_amd/csrc/sf_stages.h"

extern "C" {

int hostemu_sizeof_mesh_objective_args() { return (int)sizeof(smplfit_mesh_objective_args); }

// n triples: v, t (n, 3), sw (n) = scale * weight -> g (n, 3) cotangents, term (n) loss terms
void hostemu_mesh_objective_vertex(const float* v, const float* t, const float* sw, int n, float* g, float* term) {
  for (int i = 0; i < n; ++i) term[i] = sf::mesh_objective_vertex(v + i * 3, t + i * 3, sw[i], g + i * 3);
}

}  // extern "C"
