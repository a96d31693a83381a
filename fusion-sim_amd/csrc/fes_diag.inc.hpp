// fes_diag.inc.hpp: the energy and momentum diagnostics of a CART3D handle (fpic_energy_now, fpic_energy_record,
// fpic_energy_history) — part of fes_api.hip's translation unit (included there, inside namespace fes).  The definitions are
// the oracle's field_energy, em_field_energy and kinetic_energy (oracle/es3d_oracle.py); the kernels are fes_diag_kernels.hpp,
// the host rules (owned planes, combination of the ranks' rows) fes_diag_core.hpp, the recorder and the ranks' gather
// fes_record.inc.hpp.
//
// A reduction is enqueued on the handle's stream: one particle pass per species (kDiagBlocks partial rows each), one pass
// over the owned planes of the fields, one launch that combines the partials (a workgroup per species and one for the
// fields) and one that writes the row — to the
// handle's scratch row (fpic_energy_now) or to the recording ring (the hook diag_after_substep of fes_api.hip, after every
// `every`-th sub-step; no host synchronisation, no collective).  A rank reduces its own particles and its own planes [z0, z0 + nzl), so its LOCAL rows
// summed over the ranks count every particle and every node once.  GLOBAL on a rank with a communicator gathers the ranks'
// rows with ONE ncclAllGather and every rank combines them in rank order (fesdiag::combine): every rank gets the same
// bits, the sums of an in-process group's members in rank order, and speed_max a maximum, which a sum all-reduce cannot give.

static int diag_buffers(fpic_handle* h)
{
    Diag& g = h->es->diag;
    if (g.partial) return FPIC_OK;
    // (8-byte words: the species' partial rows, the field partials, the combined sums)
    const size_t words = static_cast<size_t>(FPIC_ENERGY_SPECIES) * kDiagBlocks * kDiagWords + 2 * kDiagFieldBlocks + FPIC_ENERGY_SPECIES * kDiagQuantities + 2;
    if (int rc = dev_alloc(h, reinterpret_cast<void**>(&g.partial), words * sizeof(double), &h->bytes_grid)) return rc;
    return dev_alloc(h, reinterpret_cast<void**>(&g.row_dev), sizeof(fpic_energy), &h->bytes_grid);
}

// the reduction of the handle's state now, its row written to `out` (device memory) on the handle's stream
template <typename T>
static int diag_enqueue(fpic_handle* h, fpic_energy* out)
{
    State* st = h->es;
    Diag& g = st->diag;
    const int nsp = static_cast<int>(st->sp.size());
    if (nsp > FPIC_ENERGY_SPECIES)
        return fail(h, FPIC_ERR_STATE, "the energy diagnostics report at most %d species (fpic_energy); this box has %d", FPIC_ENERGY_SPECIES, nsp);
    if (int rc = diag_buffers(h)) return rc;
    const Domain* d = st->dom;
    const fesdiag::Owned own = fesdiag::owned_planes(st->nz, d ? d->world : 1, d ? d->rank : 0);
    const bool yee = st->solver == FPIC_SOLVER_YEE, open = yee && st->em_open;
    if (open && d && d->halos_stale)
        return fail(h, FPIC_ERR_STATE, "the lattice fields' halo planes are stale (restored from a checkpoint): B of the integer time needs them; step once first");
    if (!fesdiag::owned_are_held(own, held_of(st), st->nz, open))
        return fail(h, FPIC_ERR_STATE, "the planes [%d, %d) this handle reduces are not all held", own.k0, own.k0 + own.nk);
    DiagScales sc{};
    unsigned long long* part = reinterpret_cast<unsigned long long*>(g.partial);
    double* fpart = g.partial + static_cast<size_t>(FPIC_ENERGY_SPECIES) * kDiagBlocks * kDiagWords;
    double* sums = fpart + 2 * kDiagFieldBlocks;
    for (int s = 0; s < nsp; ++s) {
        const Species& sp = st->sp[s];
        sc.ke[s] = 0.5 * sp.mass * st->W * kSpeedOfLight * kSpeedOfLight;
        sc.pm[s] = sp.mass * st->W * kSpeedOfLight;
        const T* a = static_cast<const T*>(sp.slab[sp.cur]);
        if (!sp.n) a = nullptr; // (nothing is read)
        diag_particles_kernel<T><<<kDiagBlocks, kDiagThreads, 0, h->stream>>>(d && a ? a : nullptr, a ? a + 3 * sp.n_pad : nullptr, a ? a + 4 * sp.n_pad : nullptr,
                                                                             a ? a + 5 * sp.n_pad : nullptr, sp.n,
                                                                             part + static_cast<size_t>(s) * kDiagBlocks * kDiagWords);
    }
    const double dv = (st->lx / st->nx) * (st->ly / st->ny) * (st->lz / st->nz);
    const double mu0 = 1.0 / (kEps0 * kSpeedOfLight * kSpeedOfLight);
    const double b0sq = st->B0[0] * st->B0[0] + st->B0[1] * st->B0[1] + st->B0[2] * st->B0[2];
    sc.e = 0.5 * kEps0 * dv;
    sc.b = yee ? 0.5 / mu0 * dv : 0.0;
    sc.b_ext = yee ? 0.5 / mu0 * b0sq * dv * (static_cast<double>(st->nx) * st->ny * own.nk) : 0.0;
    sc.substep = g.substep;
    sc.nsp = nsp;
    sc.nblk = kDiagBlocks;
    sc.nblk_f = kDiagFieldBlocks;
    const EmCoef<T> co(h);
    diag_field_kernel<T><<<kDiagFieldBlocks, kDiagThreads, 0, h->stream>>>(static_cast<const T*>(yee ? st->Ey : st->E4), yee && !open ? static_cast<const T*>(st->By) : nullptr,
                                                                         open ? static_cast<const T*>(st->Bh[st->bh_cur]) : nullptr, st->nx, st->ny, st->nz, own.k0,
                                                                         own.nk, held_of(st), co.cb[0], co.cb[1], co.cb[2], fpart);
    diag_combine_kernel<<<nsp + 1, kDiagThreads, 0, h->stream>>>(part, fpart, nsp, kDiagBlocks, kDiagFieldBlocks, sums);
    diag_row_kernel<<<1, 1, 0, h->stream>>>(sums, sc, out);
    HIP_TRY(h, hipGetLastError());
    return FPIC_OK;
}

int energy_now(fpic_handle* h, int scope, fpic_energy* out)
{
    if (!out) return fail(h, FPIC_ERR_INVALID_ARG, ".out <- Non-optional property is undefined!");
    bool collective = false;
    if (int rc = diag_scope(h, scope, collective)) return rc;
    if (!h->es->fields_ready) return fail(h, FPIC_ERR_STATE, "energy before precalc(): the fields of the current particle positions have not been computed");
    Diag& g = h->es->diag;
    if (int rc = diag_buffers(h)) return rc;
    if (int rc = h->prec == FPIC_F32 ? diag_enqueue<float>(h, g.row_dev) : diag_enqueue<double>(h, g.row_dev)) return rc;
    fpic_energy mine;
    HIP_TRY(h, hipMemcpyAsync(&mine, g.row_dev, sizeof(mine), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (!collective) {
        *out = mine;
        return FPIC_OK;
    }
    std::vector<unsigned char> all;
    if (int rc = diag_gather(h, &mine, sizeof(mine), all)) return rc;
    fesdiag::combine(reinterpret_cast<const fpic_energy*>(all.data()), 1, h->comm->world, out);
    return FPIC_OK;
}

static_assert(sizeof(fpic_energy) % sizeof(double) == 0, "a recorder's rows are whole 8-byte words");

int energy_record(fpic_handle* h, int every, uint32_t capacity)
{
    if (int rc = rec_check(h, every, capacity)) return rc;
    State* st = h->es;
    if (every > 0 && st->sp.size() > static_cast<size_t>(FPIC_ENERGY_SPECIES))
        return fail(h, FPIC_ERR_STATE, "the energy diagnostics report at most %d species (fpic_energy); this box has %zu", FPIC_ENERGY_SPECIES, st->sp.size());
    Recorder& r = st->diag.rec[kRecEnergy];
    if (int rc = rec_disarm(h, r, false)) return rc;
    if (!every) return FPIC_OK;
    if (int rc = diag_buffers(h)) return rc;
    return rec_arm(h, r, every, capacity, sizeof(fpic_energy));
}

int energy_history(fpic_handle* h, int scope, fpic_energy* rows, uint64_t capacity, uint64_t* n, uint64_t* dropped)
{
    Recorder& r = h->es->diag.rec[kRecEnergy];
    Drain d;
    if (int rc = rec_drain(h, r, scope, !rows, capacity, nullptr, n, dropped, d)) return rc;
    if (d.query) return FPIC_OK;
    const fpic_energy* mine = reinterpret_cast<const fpic_energy*>(d.rows.data());
    if (d.cnt && d.collective) {
        std::vector<unsigned char> all;
        if (int rc = diag_gather(h, mine, d.cnt * sizeof(fpic_energy), all)) return rc;
        const fpic_energy* parts = reinterpret_cast<const fpic_energy*>(all.data());
        for (uint64_t i = 0; i < d.cnt; ++i) fesdiag::combine(parts + i, d.cnt, h->comm->world, rows + i);
    } else if (d.cnt) {
        std::memcpy(rows, mine, d.cnt * sizeof(fpic_energy));
    }
    rec_drained(r, d, nullptr, n, dropped);   // (an energy row carries its sub-step)
    return FPIC_OK;
}
