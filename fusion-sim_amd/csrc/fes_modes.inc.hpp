// fes_modes.inc.hpp: the modes diagnostic of a CART3D handle (fpic_modes_now, fpic_modes_record, fpic_modes_history) — part
// of fes_api.hip's translation unit (included there after fes_series.inc.hpp, inside namespace fes).  The rules are
// fes_modes_core.hpp, the two passes fes_modes_kernels.hpp.
//
// A request is checked, its wave vectors reduced and the three twiddle tables built on the host once (modes_upload), and kept
// on the device in one allocation together with the workgroups' partial rows.  A row is enqueued on the handle's stream: the
// partial pass over the planes this handle owns, then the combine pass, which writes the row — to a scratch row
// (fpic_modes_now) or to the recording ring (the hook modes_after_substep, driven by diag_after_substep; no host
// synchronisation, no collective).  GLOBAL on a rank with a communicator gathers the ranks' rows with diag_gather and every
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
static int modes_deliver(fpic_handle* h, const std::vector<double>& mine, size_t count, bool collective, double* out)
{
    if (!count) return FPIC_OK;
    if (!collective) {
        std::memcpy(out, mine.data(), count * sizeof(double));
        return FPIC_OK;
    }
    std::vector<unsigned char> all;
    if (int rc = diag_gather(h, mine.data(), count * sizeof(double), all)) return rc;
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
    void* row = nullptr;
    std::vector<double> mine;
    if (rc == FPIC_OK) rc = dev_alloc(h, &row, q.width() * sizeof(double), nullptr);
    if (rc == FPIC_OK) rc = f32 ? modes_enqueue<float>(h, q, static_cast<double*>(row)) : modes_enqueue<double>(h, q, static_cast<double*>(row));
    if (rc == FPIC_OK) {
        mine.resize(q.width());
        hipError_t e = hipMemcpyAsync(mine.data(), row, mine.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = fail(h, FPIC_ERR_HIP, "modes read-back failed: %s", hipGetErrorString(e));
    }
    if (rc == FPIC_OK) rc = modes_deliver(h, mine, mine.size(), collective, out);
    if (row) (void)hipFree(row);
    if (int rc2 = modes_free(h, q)) return rc ? rc : rc2;
    return rc;
}

int modes_record(fpic_handle* h, const fpic_modes_spec* spec, int every, uint32_t capacity)
{
    if (every < 0) return fail(h, FPIC_ERR_INVALID_ARG, ".every <- must be >= 0 (0 turns recording off)");
    if (every > 0 && capacity < 1) return fail(h, FPIC_ERR_INVALID_ARG, ".capacity <- must be at least 1");
    if (every > 0 && !spec) return fail(h, FPIC_ERR_INVALID_ARG, ".spec <- Non-optional property is undefined!");
    ModesReq q;
    if (every > 0) // (a refused request leaves the recorder as it was)
        if (int rc = modes_upload(h, *spec, q)) return rc;
    Modes& s = h->es->diag.modes;
    if (s.ring_dev || s.req.block) HIP_TRY(h, hipStreamSynchronize(h->stream)); // (recorded rows still in flight write to it)
    if (s.ring_dev) {
        HIP_TRY(h, hipFree(s.ring_dev));
        h->bytes_grid -= s.ring.cap * s.req.width() * sizeof(double);
        s.ring_dev = nullptr;
    }
    if (int rc = modes_free(h, s.req)) return rc;
    s.ring = fesdiag::Ring();
    s.ring_substep.clear();
    s.every = 0;
    if (!every) return FPIC_OK;
    s.req = q;
    if (int rc = dev_alloc(h, reinterpret_cast<void**>(&s.ring_dev), static_cast<size_t>(capacity) * q.width() * sizeof(double), &h->bytes_grid)) {
        (void)modes_free(h, s.req);
        return rc;
    }
    s.ring.cap = capacity;
    s.ring_substep.assign(capacity, 0);
    s.every = every;
    return FPIC_OK;
}

int modes_history(fpic_handle* h, int scope, uint64_t* substeps, double* out, uint64_t capacity, uint64_t* n, uint64_t* dropped)
{
    if (!n) return fail(h, FPIC_ERR_INVALID_ARG, ".n <- Non-optional property is undefined!");
    bool collective = false;
    if (int rc = diag_scope(h, scope, collective)) return rc;
    Modes& s = h->es->diag.modes;
    uint64_t first = 0, cnt = 0, drop = 0;
    if (s.ring_dev) s.ring.pending(first, cnt, drop);
    if (!substeps) { // a query: nothing is drained
        *n = cnt;
        if (dropped) *dropped = drop;
        return FPIC_OK;
    }
    if (capacity < cnt) return fail(h, FPIC_ERR_INVALID_ARG, ".capacity <- %llu rows are pending, room for %llu", static_cast<unsigned long long>(cnt), static_cast<unsigned long long>(capacity));
    if (cnt && !out) return fail(h, FPIC_ERR_INVALID_ARG, ".out <- Non-optional property is undefined!");
    const size_t W = s.req.width();
    std::vector<double> mine(cnt * W);
    uint64_t slot[2], len[2];
    const int nr = s.ring.runs(first, cnt, slot, len);
    for (int k = 0, at = 0; k < nr; at += static_cast<int>(len[k]), ++k)
        HIP_TRY(h, hipMemcpyAsync(mine.data() + at * W, s.ring_dev + slot[k] * W, len[k] * W * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (collective) { // every rank must drain the same rows: agreed first, as fpic_energy_history does
        const double mine_n[2] = { static_cast<double>(cnt), static_cast<double>(drop) };
        std::vector<unsigned char> all;
        if (int rc = diag_gather(h, mine_n, sizeof(mine_n), all)) return rc;
        const double* ns = reinterpret_cast<const double*>(all.data());
        for (int r = 0; r < h->comm->world; ++r)
            if (ns[2 * r] != mine_n[0] || ns[2 * r + 1] != mine_n[1])
                return fail(h, FPIC_ERR_STATE, "the ranks hold different numbers of recorded rows (%llu here, %.0f on rank %d): record with the same settings on every rank",
                            static_cast<unsigned long long>(cnt), ns[2 * r], r);
    }
    if (int rc = modes_deliver(h, mine, mine.size(), collective, out)) return rc;
    for (uint64_t i = 0; i < cnt; ++i) substeps[i] = s.ring_substep[s.ring.slot(first + i)];
    s.ring.drained = s.ring.seq;
    *n = cnt;
    if (dropped) *dropped = drop;
    return FPIC_OK;
}

// the recording hook (called by diag_after_substep, which has counted the sub-step)
static int modes_after_substep(fpic_handle* h)
{
    Diag& g = h->es->diag;
    Modes& s = g.modes;
    if (!s.every || g.substep % static_cast<uint64_t>(s.every)) return FPIC_OK;
    const uint64_t slot = s.ring.slot(s.ring.seq);
    double* row = s.ring_dev + slot * s.req.width();
    if (int rc = h->prec == FPIC_F32 ? modes_enqueue<float>(h, s.req, row) : modes_enqueue<double>(h, s.req, row)) return rc;
    s.ring_substep[slot] = g.substep;
    s.ring.seq++;
    return FPIC_OK;
}
