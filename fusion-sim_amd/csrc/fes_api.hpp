// fes_api.hpp — the CART3D electrostatic extension behind the C ABI (fes_api.hip); the entry
// points of fpic_api.hip forward here when spec.geometry == FPIC_GEOM_CART3D.  Not part of the ABI.
#pragma once

#include "fpic_handle.hpp"

namespace fes {

int create(fpic_handle* h);
void release(fpic_handle* h);
int add_species(fpic_handle* h, double mass, double charge, uint64_t count, int* index);
int set_particles(fpic_handle* h, int species, const void* pos_aos, const void* vel_aos, uint64_t first, uint64_t n, int dtype);
uint64_t species_count(const fpic_handle* h, int species);
int get_particles(fpic_handle* h, int species, void* pos_aos, void* vel_aos, int dtype, uint64_t first = 0, uint64_t n = ~0ull, uint64_t stride = 1);
int get_cells(fpic_handle* h, int species, int32_t* cells, uint64_t first = 0, uint64_t n = ~0ull, uint64_t stride = 1);
int add_b(fpic_handle* h, double bx, double by, double bz);
int set_field3(fpic_handle* h, int which, const void* data, int nx, int ny, int nz, int dtype);
int read_field3(fpic_handle* h, int which, void* out, int dtype);
int precalc(fpic_handle* h);
int density(fpic_handle* h);
int substeps(fpic_handle* h, int nsub); // (step(n) = substeps(2 n))
int sort(fpic_handle* h);
int device_buffer(fpic_handle* h, int which, void** dptr, size_t* bytes);
int save_checkpoint(fpic_handle* h, const char* path);
int load_checkpoint(fpic_handle* h, const char* path);
// z-slab decomposition
int domain_init(fpic_handle* h, int rank, int world, int ghost_planes, int migrate_every, int distributed_solve);
int domain_set_particles(fpic_handle* h, int species, uint64_t n, const void* pos_aos, const void* vel_aos, uint32_t first_id, int dtype);
int domain_get_particles(fpic_handle* h, int species, void* pos_aos, void* vel_aos, uint32_t* ids, uint64_t capacity, uint64_t* n_out, int dtype);
int domain_stats(fpic_handle* h, uint64_t* migrated, uint64_t* lost);
bool is_decomposed(const fpic_handle* h);
int group_run(fpic_handle** hs, int n, int what /* 0 precalc, 1 step, 2 density */, int ncalls);
uint64_t particle_count(const fpic_handle* h);
// energy diagnostics (fes_diag.inc.hpp)
int energy_now(fpic_handle* h, int scope, fpic_energy* out);
int energy_record(fpic_handle* h, int every, uint32_t capacity);
int energy_history(fpic_handle* h, int scope, fpic_energy* rows, uint64_t capacity, uint64_t* n, uint64_t* dropped);
// phase-space histograms (fes_hist.inc.hpp)
int histogram(fpic_handle* h, const fpic_hist_spec* spec, int scope, uint64_t* counts, uint64_t* outside);
// particle selection (fes_select.inc.hpp)
int select(fpic_handle* h, const fpic_select_spec* spec, int scope, uint64_t capacity, uint32_t* ids, void* pos_aos, void* vel_aos, int dtype, uint64_t* matched);
// particle loader (fes_load.inc.hpp)
int load(fpic_handle* h, const fpic_load_spec* spec, uint64_t* loaded);
int load_profile(fpic_handle* h, const fpic_load_spec* spec, const struct fpic_load_profile* profile, uint64_t* loaded);
int load_radial(fpic_handle* h, const fpic_load_spec* spec, const struct fpic_load_radial* radial, uint64_t* loaded);
// Monte Carlo collisions with a prescribed background (fes_collide.inc.hpp)
int collide(fpic_handle* h, const fpic_collide_spec* spec, fpic_collide_result* out);
int collide_register(fpic_handle* h, const fpic_collide_spec* spec, int every, int* index);
int collide_stats(fpic_handle* h, int index, int scope, fpic_collide_result* out);
int collide_clear(fpic_handle* h);
// prescribed external forces (fes_force.inc.hpp)
int force(fpic_handle* h, const fpic_force_spec* spec, fpic_force_result* out);
int force_register(fpic_handle* h, const fpic_force_spec* spec, int* index);
int force_stats(fpic_handle* h, int index, int scope, fpic_force_result* out);
int force_clear(fpic_handle* h);
// windowed background collisions with a tabulated cross-section (fes_gas.inc.hpp)
int gas(fpic_handle* h, const fpic_gas_spec* spec, fpic_gas_result* out);
int gas_register(fpic_handle* h, const fpic_gas_spec* spec, int every, int* index);
int gas_stats(fpic_handle* h, int index, int scope, fpic_gas_result* out);
int gas_clear(fpic_handle* h);
// absorbing particle sinks and the renumbering of a thinned species (fes_remove.inc.hpp)
int remove(fpic_handle* h, const fpic_remove_spec* spec, fpic_remove_result* out);
int remove_register(fpic_handle* h, const fpic_remove_spec* spec, int every, int* index);
int remove_stats(fpic_handle* h, int index, int scope, fpic_remove_result* out);
int remove_clear(fpic_handle* h);
int renumber(fpic_handle* h, int species, uint64_t* n);
// particle sources, the capacity they grow into and the population's numbers (fes_inject.inc.hpp)
int reserve(fpic_handle* h, int species, uint64_t capacity, uint64_t* capacity_out);
int population(fpic_handle* h, int species, uint64_t* n, uint64_t* capacity, uint64_t* id_span);
int inject(fpic_handle* h, const fpic_inject_spec* spec, fpic_inject_result* out);
int inject_register(fpic_handle* h, const fpic_inject_spec* spec, int every, int* index);
int inject_stats(fpic_handle* h, int index, int scope, fpic_inject_result* out);
int inject_clear(fpic_handle* h);
// electron-impact ionisation of a background gas (fes_ionize.inc.hpp)
int ionize(fpic_handle* h, const fpic_ionize_spec* spec, fpic_ionize_result* out);
int ionize_register(fpic_handle* h, const fpic_ionize_spec* spec, int every, int* index);
int ionize_stats(fpic_handle* h, int index, int scope, fpic_ionize_result* out);
int ionize_clear(fpic_handle* h);
// fusion burn: reactants consumed, products born (fes_burn.inc.hpp)
int burn(fpic_handle* h, const fpic_burn_spec* spec, fpic_burn_result* out);
int burn_register(fpic_handle* h, const fpic_burn_spec* spec, int every, int* index);
int burn_stats(fpic_handle* h, int index, int scope, fpic_burn_result* out);
int burn_clear(fpic_handle* h);
// binary Coulomb collisions between the species of the box (fes_pair.inc.hpp)
int pair(fpic_handle* h, const fpic_pair_spec* spec, fpic_pair_result* out);
int pair_register(fpic_handle* h, const fpic_pair_spec* spec, int every, int* index);
int pair_stats(fpic_handle* h, int index, int scope, fpic_pair_result* out);
int pair_clear(fpic_handle* h);
// fusion yield tallies between the species of the box (fes_fusion.inc.hpp)
int fusion(fpic_handle* h, const fpic_fusion_spec* spec, fpic_fusion_result* out, int64_t* grid);
int fusion_register(fpic_handle* h, const fpic_fusion_spec* spec, int every, int* index);
int fusion_stats(fpic_handle* h, int index, int scope, fpic_fusion_result* out);
int fusion_grid(fpic_handle* h, int index, int64_t* grid, int reset);
int fusion_clear(fpic_handle* h);
// fusion product spectra (fes_fusion_spectrum.inc.hpp)
int fusion_spectrum(fpic_handle* h, const fpic_fusion_spectrum_spec* spec, fpic_fusion_result* out, uint64_t* words);
int fusion_spectrum_register(fpic_handle* h, const fpic_fusion_spectrum_spec* spec, int every, int* index);
int fusion_spectrum_read(fpic_handle* h, int index, fpic_fusion_result* out, uint64_t* words, int reset);
int fusion_spectrum_clear(fpic_handle* h);
// fluid moment grids (fes_mom.inc.hpp)
int moments(fpic_handle* h, const fpic_moments_spec* spec, int scope, int64_t* out, fpic_moments_info* info);
// field points and tracer particles as rows (fes_series.inc.hpp)
int series_now(fpic_handle* h, const fpic_series_spec* spec, int scope, double* points_out, double* tracers_out);
int series_record(fpic_handle* h, const fpic_series_spec* spec, int every, uint32_t capacity);
int series_history(fpic_handle* h, int scope, uint64_t* substeps, double* points_out, double* tracers_out, uint64_t capacity, uint64_t* n, uint64_t* dropped);
// Fourier amplitudes of the node fields at chosen wave vectors (fes_modes.inc.hpp)
int modes_now(fpic_handle* h, const fpic_modes_spec* spec, int scope, double* out);
int modes_record(fpic_handle* h, const fpic_modes_spec* spec, int every, uint32_t capacity);
int modes_history(fpic_handle* h, int scope, uint64_t* substeps, double* out, uint64_t capacity, uint64_t* n, uint64_t* dropped);
uint64_t last_spill(const fpic_handle* h); // out-of-window deposits of the sub-step before last (lagged read-back)

} // namespace fes
