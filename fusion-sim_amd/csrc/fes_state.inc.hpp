// fes_state.inc.hpp: the state of a CART3D handle (Species, State) and of its z-slab decomposition (Domain) — part of fes_api.hip's translation unit (included there, inside namespace fes; not a header of its own:
// the pieces share the anonymous namespace's templates).  Split out in round 5 without changing a symbol.

struct Species {
    double mass = 0, charge = 0;
    int Z = 1;
    size_t n = 0;     // particles held now (a decomposed run gains and loses particles by migration)
    size_t cap = 0;   // capacity of the arrays
    size_t n_pad = 0;
    void* slab[2] = {};
    uint32_t* id[2] = {};
    int cur = 0;
    // two bin tables: [wl] describes the live particle order, [wl ^ 1] is laid out by the next binning
    // (which may be the next push, see rebin_pending)
    uint32_t *tile_count = nullptr, *tile_cursor = nullptr;
    // a migration rides on the next re-binning push: arrivals appended at [tail_first, tail_first + tail_count) of the
    // current set, n_after = the population once that push has compacted the set
    size_t tail_first = 0, tail_count = 0, n_after = 0;
    bool ids_identity = true;   // slot s still holds the caller's particle s (no binning yet): uploads go straight to their slots
    uint32_t *tile_start2[2] = {}, *nwork2[2] = {};
    BlockWork* work2[2] = {};
    int wl = 0;
    size_t work_cap = 0;
    bool binned = false;
    bool census_fresh = false;  // tile_count holds the census of the current positions (written by the last push)
    bool rebin_pending = false; // tables [wl ^ 1] are laid out from that census: the next push re-bins
    bool rebin_now = false;     // the push in flight is that re-binning (a push in two parts decides once)
    uint32_t* chunk_census = nullptr;  // 27 words per work item: the new positions of the last in-place launch by neighbour slot
    bool chunk_census_fresh = false;   // ... of the live work list and slots: the next re-binning launch need not count
    int chunk_census_form = 0;         // ... written by a whole launch (0) or by the two parts of a rank's launch (1),
                                       //     bit 1: over the joint work list of every species (State::joint_work) instead of its own
    uint64_t chunk_census_list = 0;    // ... and which build of the joint list its items are those of (State::joint_build)
    size_t chunk_census_items = 0;     // work items the census has room for
    uint64_t layout = 0;               // counts the changes of the live bin table (what a joint work list is built from)
    void* em_args = nullptr;           // EmPushArgs of the last full-EM launch, resident for the kernel's out-of-line paths
    // fpic_remove (fes_remove.inc.hpp) has taken particles out: the ids are no longer 0 .. n - 1 but lie below id_span (one past
    // the largest id the species was ever given; it does not shrink).  The caller-order calls are refused until fpic_renumber
    bool thinned = false;
    uint64_t id_span = 0;              // read through id_span_of(): n while the species is not thinned
};
inline uint64_t id_span_of(const Species& s) { return s.thinned ? s.id_span : s.n; }

// the series diagnostic (fes_series.inc.hpp): a request's copies on the device — one allocation holding the points' normalised
// coordinates (T [npoints][3]) and, per species that has tracers, the sorted ids, their entries and the bitmap filter
struct SeriesTable {
    int species;
    uint32_t m, log2bits;
    const uint32_t *sorted, *index, *filter;
};
struct SeriesReq {
    uint32_t npoints = 0, ntracers = 0;
    void* block = nullptr;
    size_t bytes = 0;
    std::vector<SeriesTable> tables;
    size_t width() const { return static_cast<size_t>(fesser::kEntry) * (static_cast<size_t>(npoints) + ntracers); }   // doubles per row
};

// the modes diagnostic (fes_modes.inc.hpp): a request's copies on the device — one allocation holding the three twiddle tables
// (complex doubles, nx + ny + nz entries), the reduced wave vectors (int32 [nmodes][3]) and the workgroups' partial rows
struct ModesReq {
    uint32_t nmodes = 0, mask = 0;
    int nq = 0;
    int place[fesmod::kQuantities] = {};
    fesmod::Shape shape{};
    void* block = nullptr;
    size_t bytes = 0;
    const double2 *wx = nullptr, *wy = nullptr, *wz = nullptr;
    const int32_t* modes = nullptr;
    double2* partial = nullptr;
    size_t width() const { return static_cast<size_t>(2) * nmodes * nq; }   // doubles per row
};

// a recorder (fes_record.inc.hpp): after every `every`-th sub-step a row of row_bytes is enqueued into a device ring; the host
// keeps the sub-step of each slot.  The energy rows, the series and the modes have one each; what a row holds is its owner's
struct Recorder {
    int every = 0;                     // 0: off
    fesdiag::Ring ring;
    void* dev = nullptr;               // [ring.cap] rows
    size_t row_bytes = 0;
    std::vector<uint64_t> substep;     // [ring.cap]
};
enum { kRecEnergy, kRecSeries, kRecModes, kRecorders };

// The registered operators (fes_ops.inc.hpp has what they share).  A family keeps one device block of tally rows:
// `rows` rows of `words` 64-bit words — row k < MAX_OPS the totals of the k-th registered operator, row MAX_OPS the call that
// is applied now, and behind it whatever rows the family's passes need for themselves — and, where its requests carry tables,
// `tab` doubles of table room per row (in the same allocation behind the words, or `apart` in one of their own).
struct OpRows {
    int words = 0;
    size_t rows = 0, tab = 0;
    bool apart = false;
    unsigned long long* dev = nullptr;
    double* tab_dev = nullptr;
    unsigned long long* row(size_t k) const { return dev + k * words; }
    double* table(size_t k) const { return tab_dev + k * tab; }
    int room(fpic_handle* h, int words_per_row, size_t nrows, size_t tab_doubles = 0, bool tab_apart = false);   // allocates once, zeroes the words
    int zero(fpic_handle* h, size_t k, size_t n = 1) const;                                                      // rows [k, k + n), in stream order
    int copy(fpic_handle* h, size_t k, uint64_t* got, size_t nwords) const;                                      // the head of row k to the host, enqueued
    int fetch(fpic_handle* h, size_t k, uint64_t* got) const;                                                    // row k to the host; waits
    void release();
};
// what every registered operator has: its period in sub-steps (a force has none and keeps 1) and the applications so far
struct OpCommon {
    int every = 1;
    uint64_t applications = 0;
};
// a family: its rows and its registered operators, in registration order
template <typename Op>
struct OpFamily {
    OpRows rows;
    std::vector<Op> ops;
};
// the families as the members of Diag, in the order in which the sub-step hook runs them (diag_after_substep of fes_api.hip
// states the order and why): member f has the hook's part f##_after_substep
#define FES_OP_FAMILIES(X) X(force) X(collide) X(gas) X(pair) X(fusion) X(fspec) X(remove) X(inject) X(ionize)
// ... and behind the nine of DESIGN 4.26 the burners, which couple a sink and a source per event and so run after
// both: the list the hook, the release and ops_registered go through
#define FES_OP_FAMILIES_ALL(X) FES_OP_FAMILIES(X) X(burn)

// what each family's operator keeps of its own, beside OpCommon
struct CollideOp : OpCommon {          // fes_collide.inc.hpp
    fpic_collide_spec spec;
};
struct ForceOp : OpCommon {            // fes_force.inc.hpp: the request (its table pointers are not kept), the host's copy of the
    fpic_force_spec spec;              // envelope table, where its taper tables lie on the device
    std::vector<double> envelope;
    const double* taper[3];
};
struct GasOp : OpCommon {              // fes_gas.inc.hpp: the request (its table pointers are not kept), the host's copy of the
    fpic_gas_spec spec;                // cross-sections, where its tables lie on the device
    std::vector<double> sigma;
    const double* dev_sigma;
    const double* taper[3];
};
struct PairOp : OpCommon {             // fes_pair.inc.hpp
    fpic_pair_spec spec;
};
struct FusionOp : OpCommon {           // fes_fusion.inc.hpp: the request (its table pointer is not kept: the table is on the
    fpic_fusion_spec spec;             // device), the kernel's form of it; applications: since registration or the last reset
    fesfusion::Rule rule;
};
struct FspecOp : OpCommon {            // fes_fusion_spectrum.inc.hpp: as FusionOp, with the kernel's form of the axis
    fpic_fusion_spectrum_spec spec;
    fesfusion::Rule rule;
    fesfspec::Rule axis;
};
struct RemoveOp : OpCommon {           // fes_remove.inc.hpp: the live particles the applications scanned so far (the other
    fpic_remove_spec spec;             // totals are the row on the device)
    uint64_t scanned = 0;
};
struct InjectOp : OpCommon {           // fes_inject.inc.hpp
    fpic_inject_spec spec;
};
struct IonizeOp : OpCommon {           // fes_ionize.inc.hpp: as GasOp
    fpic_ionize_spec spec;
    std::vector<double> sigma;
    const double* dev_sigma;
    const double* taper[3];
};
struct BurnOp : OpCommon {             // fes_burn.inc.hpp: the request (its table pointer is not kept), the host's copy of the
    fpic_burn_spec spec;               // cross-sections, where the table lies on the device
    std::vector<double> sigma;
    const double* table;
};

// the diagnostics of a handle: the sub-step counter the recorders share, the recorders and their requests, the buffers of the
// energy reduction (fes_diag.inc.hpp), of the histograms and of the moments, the ranks' gather
struct Diag {
    uint64_t substep = 0;              // sub-steps advanced since create
    Recorder rec[kRecorders];
    SeriesReq series_req;              // what rec[kRecSeries] records (fes_series.inc.hpp)
    ModesReq modes_req;                // what rec[kRecModes] records (fes_modes.inc.hpp)
    double* partial = nullptr;         // partial rows of the species passes and of the field pass
    fpic_energy* row_dev = nullptr;    // the row of fpic_energy_now
    void* gather = nullptr;            // the ranks' rows of a collective call
    size_t gather_bytes = 0;
    unsigned long long* hist = nullptr; // the counters of fpic_histogram (fes_hist.inc.hpp): bins, then `outside`; grows to the largest request
    size_t hist_words = 0;
    unsigned long long* mom = nullptr;  // the buffer of fpic_moments (fes_mom.inc.hpp): a grid of the held planes per moment, then `rejected`, `spilled`; grows to the largest request
    size_t mom_words = 0;
    void* sel = nullptr;                // the buffer of fpic_select (fes_select.inc.hpp): the cursor, then out_id[rows], out_state[6][rows]; grows to the largest request
    size_t sel_bytes = 0;
    double* load_tab = nullptr;         // the tables of fpic_load_profile (fes_load.inc.hpp), uploaded per call; grows to the largest request
    size_t load_tab_bytes = 0;
    // the registered operators, a family each (OpFamily above); what a row holds and what lies behind row MAX_OPS is the
    // family's (its .inc.hpp)
    OpFamily<ForceOp> force;            // fesforce::kWords tally words and room for three taper tables per row
    OpFamily<CollideOp> collide;        // four count words per row
    OpFamily<GasOp> gas;                // fesgas::kWords tally words and room for the cross-section table and three taper tables per row
    OpFamily<PairOp> pair;              // eight count words per row
    OpFamily<FusionOp> fusion;          // eight count words and a table of FPIC_FUSION_TABLE_MAX doubles per row
    OpFamily<FspecOp> fspec;            // as fusion
    OpFamily<RemoveOp> remove;          // rows of kDiagWords words; behind the totals: the last application, the mark pass's counter, the move pass's partial rows
    OpFamily<InjectOp> inject;          // rows of kDiagWords words; behind the totals: the last application, the generation pass's partial rows
    OpFamily<IonizeOp> ionize;          // fesion::kWords tally words and the gas operator's table room per row; row MAX_OPS: the application in flight
    OpFamily<BurnOp> burn;              // fesburn::kWords tally words and a table of FPIC_FUSION_TABLE_MAX doubles per row; row MAX_OPS: the application in flight
    // the cell index of fpic_pair, one per side (species_a, species_b): pair_seg[s] = 4 + cells words (zeros, then per cell
    // the count -> the exclusive offset -> the end of the cell's segment), pair_index[s] = the slots by cell; both grow to
    // the largest request.  The fusion tallies and spectra use it too
    uint32_t* pair_seg[2] = {};
    uint32_t* pair_index[2] = {};
    size_t pair_seg_words[2] = {}, pair_index_words[2] = {};
    unsigned long long* fusion_grid[FPIC_FUSION_MAX_OPS + 1] = {};   // per row of `fusion` the cell grid (nx ny nz int64, allocated when the row is first used)
    OpRows fspec_bins;                  // per row of `fspec` (FPIC_FUSION_SPECTRUM_BINS_MAX + 2) x 2 words of the histogram
};
inline void diag_release(Diag& g)
{
    for (Recorder& r : g.rec)
        if (r.dev) (void)hipFree(r.dev);
    for (void* p : { g.series_req.block, g.modes_req.block, static_cast<void*>(g.partial), static_cast<void*>(g.row_dev), g.gather, static_cast<void*>(g.hist), static_cast<void*>(g.mom), g.sel, static_cast<void*>(g.load_tab),
                     static_cast<void*>(g.pair_seg[0]), static_cast<void*>(g.pair_seg[1]), static_cast<void*>(g.pair_index[0]), static_cast<void*>(g.pair_index[1]) })
        if (p) (void)hipFree(p);
#define X(f) g.f.rows.release();
    FES_OP_FAMILIES_ALL(X)
#undef X
    g.fspec_bins.release();
    for (unsigned long long* p : g.fusion_grid)
        if (p) (void)hipFree(p);
    g = Diag();
}

struct State {
    int nx = 0, ny = 0, nz = 0;
    double lx = 0, ly = 0, lz = 0, W = 1;
    size_t nodes = 0;
    // the planes the node arrays hold (fes_kernels.hpp, Held): all nz of them, or — a rank of a compact decomposition —
    // the slab with its halo: zs0 = z0 - H, nzs = nzl + 2 H + 1 planes
    int zs0 = 0, nzs = 0;
    int solver = FPIC_SOLVER_NONE;
    int ltx = FES_LTX, lty = FES_LTY, ltz = FES_LTZ; // log2 of the tile edges: 16x16x8 cells (electrostatic), 8x8x8 (full EM)
    int ntx = 0, nty = 0, ntz = 0;
    uint32_t ntiles = 0; // + 1 always-empty bin (the scan kernel's clipped bin)
    long long* rho_fixed = nullptr;
    void *rho = nullptr, *hat = nullptr, *phi = nullptr, *E4 = nullptr;
    // full EM (solver = YEE): the lattice's E and B, the node-centred B (E4 holds the node-centred E), the integer current grid
    void *Ey = nullptr, *By = nullptr, *B4n = nullptr;
    // the chained lattice step of an undecomposed full-EM handle (em_chain_kernel): B at half time, two arrays taken in turns;
    // em_open: Ey is E of the integer time reached, Bh[bh_cur] is B half a step before it, By is stale until em_close()
    void* Bh[2] = { nullptr, nullptr };
    int bh_cur = 0;
    bool em_open = false;
    long long* Jfix = nullptr;
    double* k2[3] = {};
    rocfft_plan fwd = nullptr, inv = nullptr;
    rocfft_execution_info info_f = nullptr, info_i = nullptr;
    void *work_f = nullptr, *work_i = nullptr;
    double B0[3] = { 0, 0, 0 };
    unsigned long long* spilled = nullptr;
    // the work list of a launch that pushes every binned species (Push3Joint): items (tile, k), rebuilt when a species'
    // bin table has changed
    fpic::BlockWork* joint_work = nullptr;
    uint32_t* joint_nwork = nullptr;
    size_t joint_cap = 0;
    std::vector<std::pair<size_t, uint64_t>> joint_built_from; // (species, layout) of the list in joint_work
    uint64_t joint_build = 0;          // counts the rebuilds (a per-item census belongs to the list it was written over)
    bool joint_now = false;            // the two parts of one sub-step's launch use the same list
    unsigned long long* spilled_host = nullptr; // pinned, 2 lagged slots
    hipEvent_t spill_event[2] = {};
    bool spill_pending[2] = {};
    unsigned long long spill_seq = 0, last_spill = 0;
    int substeps_since_bin = 0;
    bool fields_ready = false;
    // power-of-two grids: the Poisson solve runs on the library's own FFT passes (fes_fft.hpp), which read the integer
    // charge grid directly; rho (T) is then formed only when somebody reads it
    bool own_fft = false, rho_fresh = true;
    void* fft_tw[3] = {};   // twiddle tables exp(-2 pi i t / n) of the three axes (T pairs)
    std::vector<Species> sp;
    struct Domain* dom = nullptr; // z-slab decomposition over several GPUs (fpic_domain_init)
    Diag diag;
};

// the refusal of a call that addresses particles in the caller's order (get / set particles and cells, the loaders, the
// checkpoint, the decomposition) on a species fpic_remove has thinned: those paths scatter by id into arrays of n entries
inline int refuse_thinned(fpic_handle* h, const Species& s, const char* name)
{
    if (!s.thinned) return FPIC_OK;
    return fail(h, FPIC_ERR_STATE, "%s addresses particles in the caller's order, and species %d has lost particles to fpic_remove: its %zu ids are no longer 0 .. n-1 (they lie below %llu); read it with fpic_select, or call fpic_renumber first",
                name, static_cast<int>(&s - h->es->sp.data()), s.n, static_cast<unsigned long long>(s.id_span));
}

// Spatial decomposition: rank r of `world` owns the particles whose cell lies in the
// planes [z0, z0 + nzl) and G ghost planes on either side, in which its particles may still sit and deposit
// until the next migration.  Per sub-step: ghost-plane reduce of the int64 charge grid with the two
// neighbours (exact), all-gather of the owned planes of rho, the field solve on every rank; every
// `migrate_every` sub-steps the particles that left the slab move to the neighbour that owns them.
struct Domain {
    int rank = 0, world = 1, G = 2, nzl = 0, z0 = 0;
    int migrate_every = 4;
    int substeps_since_migration = 0;
    long long* ghost_recv[2] = {};      // [0]: from the slab above (its lower ghost planes, G), [1]: from below (G + 1)
    void* mig_send[2] = {};             // [0]: to the slab below, [1]: to the slab above
    void* mig_recv[2] = {};             // [0]: from above, [1]: from below
    unsigned mig_cap = 0;               // records per buffer
    // full EM: halo planes of the lattice fields / ghost planes of the current on each side (G + 2), and where the
    // neighbours' current ghost planes arrive (3 int64 per node)
    int H = 0;
    long long* j_recv[2] = {};
    bool halos_stale = false;           // lattice fields restored from a checkpoint: the halo planes are refreshed before the next sub-step
    // per species a block of 8 words: down, up, lost, overflow | received from above, from below | -, - ; after the
    // kMigSpecies blocks one more, whose first word is the ranks' agreement (agree_max)
    unsigned* counts_dev = nullptr;
    unsigned* counts_host = nullptr;    // pinned copy
    int mig_sp = 0;                     // the species whose payload the exchange X_MIG_PAYLOAD moves
    // the ghost-plane exchange of a sub-step runs on a stream of its own while the interior of the slab is pushed
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_boundary = nullptr, ev_ghost = nullptr;
    bool overlap = true;                // FPIC_DOMAIN_OVERLAP=0: everything on the handle's stream, one launch per species
    bool em_chain = true, em_chain_agreed = false; // FPIC_EM_CHAIN=0 (read by fpic_domain_init, agreed by the ranks before the first full-EM sub-step)
    // TEST SWITCH (FPIC_TEST_FAULT, read by fpic_domain_init; tests/test_gpu_fake_rccl.py's negative controls): bit 0 drops the
    // wait of the communicator's stream for the handle's stream (comm_fork), bit 1 the wait of the handle's stream for the
    // exchange (comm_join) — the two dependencies a stream-ordered transport must show as wrong bits when they are missing
    int test_fault = 0;
    uint64_t migrated = 0, lost = 0, deferred = 0; // deferred: leavers that did not fit a message and left with a later one
    // slab-decomposed Poisson solve (distributed = true): 2-D transforms of the owned planes, transpose over the ranks,
    // transforms along z of the rank's share of the ky rows, and back; otherwise every rank transforms the whole grid
    bool distributed = false;
    int nyl = 0;
    int phi_below = 0, phi_above = 0;   // planes of the potential a rank receives from its neighbours after the decomposed solve
    void *hatA = nullptr, *hatB = nullptr, *xbuf = nullptr; // [nzl][ny][nxh], [nz][nyl][nxh], transposition staging (complex T each)
    rocfft_plan p2f = nullptr, p2i = nullptr, pzf = nullptr, pzi = nullptr;
    rocfft_execution_info i2f = nullptr, i2i = nullptr, izf = nullptr, izi = nullptr;
    void* fft_work[4] = {};
    void* hatZ = nullptr;               // hatB turned to [nyl * nxh][nz]: the z pass is contiguous there
    // distributed_solve = 2 (fes_tri.hpp): no transposition — the decomposed direction is a periodic tridiagonal system per
    // (kx, ky) mode, reduced per rank to two interface planes; tri = [world][2 planes of the half spectrum + nzl values of
    // the (0, 0) mode's line] (complex T), all-gathered in place; tri_block = complex values per rank
    bool interface_solve = false;
    void* tri = nullptr;
    size_t tri_block = 0;
};
