// fes_modes.inc.hpp: the modes diagnostic of a CART3D handle (fpic_modes_now, fpic_modes_record, fpic_modes_history) — part
// of fes_api.hip's translation unit (included there after fes_series.inc.hpp, inside namespace fes).  The rules are
// fes_modes_core.hpp, the two passes fes_modes_kernels.hpp.
//
// A request is checked, its wave vectors reduced and the three twiddle tables built on the host once (modes_upload), and kept
// on the device in one allocation together with the workgroups' partial rows.  A row is enqueued on the handle's stream: the
// partial pass over the planes this handle owns, then the combine pass, which writes the row — to a scratch row
// (fpic_modes_now) or to the recording ring (the hook diag_after_substep; no host synchronisation, no collective; the
// recorder is fes_record.inc.hpp).  GLOBAL on a rank with a communicator gathers the ranks' rows with diag_gather and every
// rank adds them in rank order (fesmod::add_parts).
//
// What the arrays hold on the owned planes when a row is taken (a call, or the hook at the end of a sub-step): E4 / B4n are
// what a point row of the series reads; the integer charge grid is complete there in every mode — an undecomposed handle
// deposits the whole grid, a rank of a decomposition has added its neighbours' ghost planes (dom_fields, dom_density) on the
// handle's stream before the hook runs, whichever Poisson solve follows — so no mode refuses FPIC_MODE_RHO.

static int modes_free(fpic_handle* h, ModesReq& q)
{
    if (q.block) {
        HIP_TRY(h, hipFree(q.block));
        h->bytes_grid -= q.bytes;
    }
    q = ModesReq();
    return FPIC_OK;
}

// the dynamic LDS of the partial pass: the x table if it is short enough, the staged segment (or the 256 complex numbers of
// the closing sum, whichever is longer) — at most 32 KiB + 16 KiB, below the 64 KiB a launch gets without asking
static size_t modes_lds_bytes(const ModesReq& q, int nx)
{
    const size_t stage = std::max<size_t>(static_cast<size_t>(q.nq) * fesmod::kSegment * sizeof(double), fesmod::kThreads * sizeof(double2));
    return (nx <= fesmod::kWxLdsMax ? static_cast<size_t>(nx) * sizeof(double2) : 0) + stage;
}

// checks `spec` against the handle and builds its device copies into `q` (empty before)
static int modes_upload(fpic_handle* h, const fpic_modes_spec& spec, ModesReq& q)
{
    State* st = h->es;
    if (const char* why = fesmod::check(spec, st->nx, st->ny, st->nz)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (!st->fields_ready) return fail(h, FPIC_ERR_STATE, "modes before precalc(): the fields of the current particle positions have not been computed");
    const Domain* d = st->dom;
    const fesdiag::Owned own = fesdiag::owned_planes(st->nz, d ? d->world : 1, d ? d->rank : 0);
    if (!fesdiag::owned_are_held(own, held_of(st), st->nz, false))
        return fail(h, FPIC_ERR_STATE, "the planes [%d, %d) this handle sums are not all held", own.k0, own.k0 + own.nk);
    q.nmodes = spec.nmodes;
    q.mask = spec.mask;
    q.nq = fesmod::places(spec.mask, q.place);
    q.shape = fesmod::shape(spec.nmodes, static_cast<uint64_t>(own.nk) * st->ny);
    // the block: wx, wy, wz (complex doubles), the reduced wave vectors (padded to 16 bytes), the partial rows
    const int n[3] = { st->nx, st->ny, st->nz };
    const size_t tw = (static_cast<size_t>(n[0]) + n[1] + n[2]) * sizeof(double2);
    const size_t mv = (static_cast<size_t>(spec.nmodes) * 3 * sizeof(int32_t) + 15) / 16 * 16;
    const size_t part = static_cast<size_t>(q.shape.blocks) * q.width() * sizeof(double);
    std::vector<unsigned char> host(tw + mv, 0);
    double* w = reinterpret_cast<double*>(host.data());
    for (int a = 0; a < 3; ++a) {
        const std::vector<double> t = fesmod::table(n[a]);
        std::memcpy(w, t.data(), t.size() * sizeof(double));
        w += t.size();
    }
    int32_t* mr = reinterpret_cast<int32_t*>(host.data() + tw);
    for (uint32_t m = 0; m < spec.nmodes; ++m)
        for (int a = 0; a < 3; ++a) mr[3 * m + a] = fesmod::reduce(spec.modes[3 * m + a], n[a]);
    void* block = nullptr;
    if (int rc = dev_alloc(h, &block, host.size() + part, &h->bytes_grid)) return rc;
    q.block = block;
    q.bytes = host.size() + part;
    unsigned char* base = static_cast<unsigned char*>(block);
    q.wx = reinterpret_cast<const double2*>(base);
    q.wy = q.wx + n[0];
    q.wz = q.wy + n[1];
    q.modes = reinterpret_cast<const int32_t*>(base + tw);
    q.partial = reinterpret_cast<double2*>(base + tw + mv);
    // (synchronous: the staging vector goes out of scope)
    hipError_t e = hipMemcpyAsync(block, host.data(), host.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)modes_free(h, q);
        return fail(h, FPIC_ERR_HIP, "the upload of a modes request failed: %s", hipGetErrorString(e));
    }
    return FPIC_OK;
}

// the row of the handle's state now, written to `row` (device memory, q.width() doubles) on the handle's stream
template <typename T>
static int modes_enqueue(fpic_handle* h, const ModesReq& q, double* row)
{
    State* st = h->es;
    const Domain* d = st->dom;
    const fesdiag::Owned own = fesdiag::owned_planes(st->nz, d ? d->world : 1, d ? d->rank : 0);
    // (a request is laid out for the planes the handle owned when it was made)
    const fesmod::Shape now = fesmod::shape(q.nmodes, static_cast<uint64_t>(own.nk) * st->ny);
    if (now.blocks != q.shape.blocks || now.rows_per_block != q.shape.rows_per_block || !fesdiag::owned_are_held(own, held_of(st), st->nz, false))
        return fail(h, FPIC_ERR_STATE, "the decomposition has changed since this modes request was made: record again");
    ModesArgs<T> a{};
    a.E4 = (q.mask & 0x0Fu) ? static_cast<const T*>(st->E4) : nullptr;
    a.B4n = (q.mask & 0x70u) ? static_cast<const T*>(st->B4n) : nullptr;
    a.rho = (q.mask & FPIC_MODE_RHO) ? st->rho_fixed : nullptr;
    const double dv = (st->lx / st->nx) * (st->ly / st->ny) * (st->lz / st->nz);
    a.rho_scale = h->spec.particle_charge * st->W / (4398046511104.0 * dv); // q0 W / (2^42 dV), as refresh_rho
    a.nx = st->nx; a.ny = st->ny; a.nz = st->nz;
    a.held = held_of(st);
    a.k0 = own.k0; a.nk = own.nk;
    a.wx = q.wx; a.wy = q.wy; a.wz = q.wz;
    a.modes = q.modes;
    a.nmodes = q.nmodes;
    a.nq = q.nq;
    for (int b = 0; b < fesmod::kQuantities; ++b) a.place[b] = q.place[b];
    a.log2p = q.shape.log2p;
    a.slots = q.shape.slots;
    a.rows_per_block = q.shape.rows_per_block;
    a.partial = q.partial;
    const size_t lds = modes_lds_bytes(q, st->nx);
    if (st->nx <= fesmod::kWxLdsMax) modes_partial_kernel<T, true><<<q.shape.blocks, fesmod::kThreads, lds, h->stream>>>(a);
    else modes_partial_kernel<T, false><<<q.shape.blocks, fesmod::kThreads, lds, h->stream>>>(a);
    const unsigned width = static_cast<unsigned>(q.width());
    modes_combine_kernel<<<width, 64, 0, h->stream>>>(reinterpret_cast<const double*>(q.partial), q.shape.blocks, width, static_cast<double>(st->nodes), row);
    HIP_TRY(h, hipGetLastError());
    return FPIC_OK;
}

// rows [rows][width] of this handle -> the caller's array, the ranks' rows added in rank order if collective
static int modes_deliver(fpic_handle* h, const double* mine, size_t count, bool collective, double* out)
{
    if (!count) return FPIC_OK;
    if (!collective) {
        std::memcpy(out, mine, count * sizeof(double));
        return FPIC_OK;
    }
    std::vector<unsigned char> all;
    if (int rc = diag_gather(h, mine, count * sizeof(double), all)) return rc;
    fesmod::add_parts(reinterpret_cast<const double*>(all.data()), count, h->comm->world, count, out);
    return FPIC_OK;
}

int modes_now(fpic_handle* h, const fpic_modes_spec* spec, int scope, double* out)
{
    if (!spec) return fail(h, FPIC_ERR_INVALID_ARG, ".spec <- Non-optional property is undefined!");
    if (!out) return fail(h, FPIC_ERR_INVALID_ARG, ".out <- Non-optional property is undefined!");
    bool collective = false;
    if (int rc = diag_scope(h, scope, collective)) return rc;
    const bool f32 = h->prec == FPIC_F32;
    ModesReq q;
    int rc = modes_upload(h, *spec, q);
    std::vector<double> mine;
    if (rc == FPIC_OK)
        rc = rec_row_now(h, q.width() * sizeof(double), "modes",
                         [&](void* row) { return f32 ? modes_enqueue<float>(h, q, static_cast<double*>(row)) : modes_enqueue<double>(h, q, static_cast<double*>(row)); }, mine);
    if (rc == FPIC_OK) rc = modes_deliver(h, mine.data(), mine.size(), collective, out);
    const int rc2 = modes_free(h, q);
    return rc ? rc : rc2;
}

int modes_record(fpic_handle* h, const fpic_modes_spec* spec, int every, uint32_t capacity)
{
    if (int rc = rec_check(h, every, capacity)) return rc;
    if (every > 0 && !spec) return fail(h, FPIC_ERR_INVALID_ARG, ".spec <- Non-optional property is undefined!");
    ModesReq q;
    if (every > 0) // (a refused request leaves the recorder as it was)
        if (int rc = modes_upload(h, *spec, q)) return rc;
    Diag& g = h->es->diag;
    Recorder& r = g.rec[kRecModes];
    if (int rc = rec_disarm(h, r, g.modes_req.block != nullptr)) return rc;
    if (int rc = modes_free(h, g.modes_req)) return rc;
    if (!every) return FPIC_OK;
    g.modes_req = q;
    const int rc = rec_arm(h, r, every, capacity, q.width() * sizeof(double));
    if (rc) (void)modes_free(h, g.modes_req);
    return rc;
}

int modes_history(fpic_handle* h, int scope, uint64_t* substeps, double* out, uint64_t capacity, uint64_t* n, uint64_t* dropped)
{
    Recorder& r = h->es->diag.rec[kRecModes];
    Drain d;
    if (int rc = rec_drain(h, r, scope, !substeps, capacity, out ? nullptr : "out", n, dropped, d)) return rc;
    if (d.query) return FPIC_OK;
    if (d.cnt)
        if (int rc = modes_deliver(h, d.rows.data(), d.rows.size(), d.collective, out)) return rc;
    rec_drained(r, d, substeps, n, dropped);
    return FPIC_OK;
}
