/*
 * empic_native.js — drop-in for the reference's `empic` module on MI355X.
 *
 *   const empic = require('./empic_native.js');
 *   const simulation = empic.makeCylindricalParticlePusher(spec);   // empic.js:30
 *   simulation.set({position, velocity, sink_mask, source_pdf});    // empic.js:1157
 *   simulation.addCurrentLoop(0.8, 2.0, -1e7);                      // empic.js:1352
 *   simulation.precalc();                                           // empic.js:1413
 *   simulation.step(); simulation.density();                        // empic.js:1436, :1471
 *
 * Same factory name, same method names, same argument meaning and the same
 * synchronous `throw new Error(".prop <- ...")` on a bad spec (utilities.js:118-127)
 * as the reference object.  The arithmetic runs in hand-written HIP kernels for
 * gfx950 behind libfusionpic.so; this file only validates, flattens nested arrays
 * into typed arrays, and forwards.  There is no JavaScript or CPU compute path: if
 * the addon or a gfx950 device is missing, the factory throws.
 *
 * What cannot exist outside a browser is `canvas` (empic.js:60).  In its place:
 *   readDensity(out?)   -> Float32Array 4*nr*nz, index 4*(i + j*nr), moments01_avgA
 *   readMoments(out?)   -> moments01;  readGrid(name, out?) for any other texture
 *   getParticles()      -> {position, velocity, rand, alive} in the caller's order
 *   setRandomState({entropy, rand}) -> reproducible runs (the reference seeds from
 *                          window.crypto and Math.random, empic.js:148-173)
 * Extension keys of spec (all optional): precision 'fp32'|'fp64', device (or devices: [d]), count,
 * compat (default true: keep quirk Q1 of empic.js:645), sort_interval, fuse_deposit
 * (default true; 'census' keeps only the tile census and re-binning in step()), rng 'reference'|'counter' + seed (counter = Philox4x32-10 per particle
 * and sub-step instead of the reference's entropy-table generator; not the reference's
 * random stream).
 * shape 'cic' replaces density()'s 11x11 sprite by a bilinear deposit on the four nearest cell centres (extension).
 * raster_subpixel_bits b (1..8) draws density()'s point sprites as a rasteriser with b sub-pixel bits does (snapped window
 * positions, cropped instead of discarded outside the target); 4 reproduces the reference under Chromium's SwiftShader bit
 * for bit, absent / 0 = ideal sprites (include/fusionpic.h).
 * geometry 'cart3d' (+ ny, length_y, solver 'poisson_fft'|'none', macro_weight) selects the self-consistent
 * electrostatic box — an extension with no reference counterpart (include/fusionpic.h): radius, height are
 * then the box lengths along x and z, nr, nz the node counts; same method names, plus addSpecies, addB,
 * readField, energy, recordEnergy, energyHistory, histogram, moments, series, recordSeries, seriesHistory, modes, recordModes, modesHistory.  Multi-GPU (one process per GPU): empic.commUniqueId() on rank 0, simulation.commInit(id,
 * rank, world) on every rank; density() then sums the per-cell sums over the ranks inside the library (RCCL).
 */
'use strict';
const path = require('path');

let native = null;
function addon() {
    if (native) return native;
    // (FUSIONPIC_NAPI_ADDON: another build of the same addon — `make -C fusion-sim_amd sanitize` points it at the ASan / UBSan build)
    const file = process.env.FUSIONPIC_NAPI_ADDON || path.join(__dirname, '..', 'lib', 'fusionpic_napi.node');
    try {
        native = require(file);
    } catch (e) {
        throw new Error('fusionpic: cannot load ' + file + ' (' + e.message +
            '); build it with `make -C fusion-sim_amd napi`. There is no CPU fallback.');
    }
    return native;
}

// ---- validate_object / validate_property (utilities.js:11-127), same messages
function validate_property(test, control) {
    if (typeof test === 'undefined') {
        if (!Array.isArray(control) || typeof control[0] !== 'undefined') {
            throw new Error(' <- Non-optional property is undefined!');
        }
    } else if (typeof test !== control) {
        if (Array.isArray(control)) {
            // utilities.js:40-49 is try/finally with no catch: the first defined alternative that does not
            // match throws straight through, later alternatives are never tried (kept, as the reference behaves)
            let failed = true;
            for (let i = 0; failed && i < control.length; i++) {
                if (typeof control[i] !== 'undefined') { validate_property(test, control[i]); failed = false; }
            }
            if (failed) throw new Error(' <- Property does not match any given possible types!');
        } else if (typeof control === 'object' && typeof test === 'object') {
            validate_object(test, control);
        } else {
            throw new Error(' <- Property does not match any given possible types!');
        }
    }
}
function validate_object(test, control) {
    for (const prop in control) {
        try { validate_property(test[prop], control[prop]); } catch (error) { throw new Error('.' + prop + error.message); }
    }
}

const GRID_IN = { E: 0, B: 1, sink_mask: 2, source_pdf: 3 };
const GRID_OUT = { moments: 0, norm: 1, avg: 2, R1: 3, R2: 4, R3: 5, A: 6, B: 7, E: 8, sink: 9, inv_cdf: 10 };

function isFloatArray(a) { return a instanceof Float32Array || a instanceof Float64Array; }

// a caller-supplied output buffer must be exactly as long as what the native call writes
function checkLength(buf, want, name) {
    if (buf !== undefined && buf !== null && buf.length !== want) {
        throw new RangeError('.' + name + ' <- expected a typed array of ' + want + ' elements, got ' + buf.length);
    }
    return buf;
}

// value[i][j][k] or value[i][j] -> Float64Array (JavaScript numbers are doubles)
function flattenGrid(value, nr, nz, ncomp, name) {
    if (isFloatArray(value)) {
        if (value.length !== nr * nz * ncomp) throw new Error('.' + name + ' <- expected ' + (nr * nz * ncomp) + ' elements');
        return value;
    }
    if (!Array.isArray(value) || value.length < nr) throw new Error('.' + name + ' <- expected [' + nr + '][' + nz + ']' + (ncomp > 1 ? '[3]' : ''));
    const out = new Float64Array(nr * nz * ncomp);
    for (let i = 0; i < nr; i++) {
        const row = value[i];
        for (let j = 0; j < nz; j++) {
            if (ncomp === 1) out[i * nz + j] = row[j];
            else for (let k = 0; k < ncomp; k++) out[(i * nz + j) * ncomp + k] = row[j][k];
        }
    }
    return out;
}

function flattenParticles(value, n, name) {
    if (isFloatArray(value)) {
        if (value.length !== 3 * n) throw new Error('.' + name + ' <- expected ' + (3 * n) + ' elements');
        return value;
    }
    if (!Array.isArray(value) || value.length < n) throw new Error('.' + name + ' <- expected [' + n + '][3]');
    const out = new Float64Array(3 * n);
    for (let p = 0; p < n; p++) { out[3 * p] = value[p][0]; out[3 * p + 1] = value[p][1]; out[3 * p + 2] = value[p][2]; }
    return out;
}

// stepAsync(ncalls) -> Promise (SURVEY 8(b), threading): the step runs on a worker thread of Node's pool; the handle is
// not thread-safe, so every other method of the simulation throws until the promise has settled.
function addStepAsync(out, lib, handle) {
    let busy = false;
    for (const name of Object.keys(out)) {
        const f = out[name];
        if (typeof f !== 'function') continue;
        out[name] = function () {
            if (busy) throw new Error('.' + name + ' <- a stepAsync() of this simulation is still running');
            return f.apply(this, arguments);
        };
    }
    out.stepAsync = function (ncalls) {
        if (busy) return Promise.reject(new Error('.stepAsync <- a stepAsync() of this simulation is still running'));
        busy = true;
        const done = () => { busy = false; };
        return lib.stepAsync(handle(), ncalls === undefined ? 1 : ncalls).then(v => { done(); return v; }, e => { done(); throw e; });
    };
    return out;
}

const FIELD3 = { E: 0, rho: 1, phi: 2, rho_fixed: 3, B: 4, edge_E: 5, face_B: 6, J_fixed: 7 };   // B, edge_E, face_B, J_fixed: full EM (solver 'yee')

// spec.geometry === 'cart3d': the electrostatic box behind the same method names
function makeBox(spec, lib) {
    validate_object(spec, { ny: 'number', length_y: 'number', solver: [, 'string'], macro_weight: [, 'number'] });
    if (spec.solver !== undefined && ['poisson_fft', 'none', 'yee'].indexOf(spec.solver) < 0) throw new Error(".solver <- must be 'poisson_fft', 'yee' or 'none'");
    const fp64 = spec.precision === 'fp64';
    const n0 = spec.count ? spec.count : spec.nparticles * spec.nparticles;
    let h = lib.create(spec.radius, spec.height, spec.nr, spec.nz, spec.dt, spec.nparticles, spec.particle_mass, spec.particle_charge,
        spec.count || 0, fp64 ? 1 : 0, spec.device || 0, 0, spec.sort_interval || 0, 0, 0, 0, 0,
        1, spec.solver === 'none' ? 0 : (spec.solver === 'yee' ? 2 : 1), spec.ny, spec.length_y, spec.macro_weight === undefined ? 1 : spec.macro_weight, 0, 0);
    const nx = spec.nr, ny = spec.ny, nz = spec.nz, nodes = nx * ny * nz;
    const counts = [n0];      // per species: the particles it holds, as last learnt; on a rank of a decomposition its capacity
    let decomposed = false;
    // the particles a species holds NOW, from the library (fpic_population): registered sources and sinks change it inside step(),
    // and the caller-order reads write that many rows.  A rank of a decomposition keeps its capacity; a library without the
    // call keeps the count last learnt
    const live = function (sp) {
        if (!decomposed) { try { counts[sp] = lib.population(h, sp).n; } catch (err) { /* the call below names what is wrong */ } }
        return counts[sp];
    };
    const Real = fp64 ? Float64Array : Float32Array;
    const out = {};
    out.addSpecies = function (mass, charge, count) { const s = lib.addSpecies(h, mass, charge, count); counts.push(count); return s; };
    out.set = function (value, species) {                                      // empic.js:1157: position [N][3] m, velocity [N][3] in c
        const sp = species || 0, n = live(sp);
        if (value.position) lib.setParticlesRange(h, sp, 0, flattenParticles(value.position, n, 'position'), null);
        if (value.velocity) lib.setParticlesRange(h, sp, 0, null, flattenParticles(value.velocity, n, 'velocity'));
        if (value.E) {
            let e = value.E;
            if (!isFloatArray(e)) {                                           // value[i][j][k][3]
                e = new Float64Array(3 * nodes);
                for (let i = 0; i < nx; i++) for (let j = 0; j < ny; j++) for (let k = 0; k < nz; k++)
                    for (let c = 0; c < 3; c++) e[3 * ((i * ny + j) * nz + k) + c] = value.E[i][j][k][c];
            }
            lib.setField3(h, FIELD3.E, checkLength(e, 3 * nodes, 'E'), nx, ny, nz);
        }
    };
    out.setRange = function (first, value, species) { lib.setParticlesRange(h, species || 0, first, value.position || null, value.velocity || null); };
    out.addBZ = function (Bz) { lib.addBZ(h, Bz); };                           // empic.js:1391
    out.addB = function (bx, by, bz) { lib.addB(h, bx, by, bz); };
    out.precalc = function () { lib.precalc(h); };                             // empic.js:1413: fields <- particles (deposit + solve)
    out.step = function (ncalls) { lib.step(h, ncalls === undefined ? 1 : ncalls); };  // empic.js:1436: 2 sub-steps
    out.substeps = function (n) { lib.substeps(h, n === undefined ? 1 : n); };         // extension: single sub-steps, step(k) = substeps(2 k)
    out.density = function () { lib.density(h); };                             // empic.js:1471: the charge density is always current
    out.readField = function (name, buf) {
        if (!(name in FIELD3)) throw new Error('.name <- unknown field ' + name);
        const len = nodes * (name === 'rho' || name === 'phi' || name === 'rho_fixed' ? 1 : (name === 'J_fixed' ? 3 : 4));
        const fresh = name === 'rho_fixed' || name === 'J_fixed' ? new BigInt64Array(len) : new Real(len);   // the exact integer grids
        return lib.readField3(h, FIELD3[name], checkLength(buf, len, 'out') || fresh);
    };
    out.getParticles = function (into, species) {
        const sp = species || 0, n = live(sp);
        const r = into || { position: new Real(3 * n), velocity: new Real(3 * n) };
        checkLength(r.position, 3 * n, 'position'); checkLength(r.velocity, 3 * n, 'velocity');
        lib.getParticlesOf(h, sp, r.position || null, r.velocity || null);
        return r;
    };
    out.getCells = function (buf, species) { const n = live(species || 0); return lib.getCellsOf(h, species || 0, checkLength(buf, n, 'cells') || new Int32Array(n)); };
    // the mirror of setRange, and a sampled read-back: the caller's particles first, first + stride, ... (count of them;
    // stride 1 = the range [first, first + count)); 2e9 particles do not fit one typed array
    out.getRange = function (first, count, into, species, stride) {
        const r = into || { position: new Real(3 * count), velocity: new Real(3 * count) };
        checkLength(r.position, 3 * count, 'position'); checkLength(r.velocity, 3 * count, 'velocity');
        lib.getParticlesRange(h, species || 0, first, stride === undefined ? 1 : stride, r.position || null, r.velocity || null);
        return r;
    };
    out.commInit = function (id, rank, world, overlap) { lib.commInit(h, id, rank, world, overlap === false ? 0 : 1); };
    out.commDestroy = function () { lib.commDestroy(h); };
    out.commInfo = function () { return lib.commInfo(h); };                  // { rank, world } as the library sees them
    // z-slab decomposition (this process = rank `rank` of `world`, after commInit with the same numbers): the rank's
    // particles arrive through domainSet with their global indices; step() then exchanges ghost planes, halos and
    // migrating particles with the neighbours inside the library
    out.domainInit = function (rank, world, options) {
        const o = options || {};
        lib.domainInit(h, rank, world, o.ghost_planes === undefined ? 2 : o.ghost_planes, o.migrate_every === undefined ? 4 : o.migrate_every,
                       o.distributed_solve === 'interface' || o.distributed_solve === 2 ? 2 : (o.distributed_solve ? 1 : 0));
        decomposed = true;      // (counts[] is the rank's capacity from now on: domainGet sizes its arrays by it)
    };
    out.domainSet = function (value, firstId, species) {
        const sp = species || 0;
        const p = isFloatArray(value.position) ? value.position : flattenParticles(value.position, value.position.length, 'position');
        const v = isFloatArray(value.velocity) ? value.velocity : flattenParticles(value.velocity, value.velocity.length, 'velocity');
        lib.domainSetParticles(h, sp, p, v, firstId || 0);
    };
    out.domainGet = function (species) {
        const sp = species || 0, cap = counts[sp];
        const position = new Real(3 * cap), velocity = new Real(3 * cap), ids = new Uint32Array(cap);
        const n = lib.domainGetParticles(h, sp, position, velocity, ids);
        return { n: n, position: position.subarray(0, 3 * n), velocity: velocity.subarray(0, 3 * n), ids: ids.subarray(0, n) };
    };
    out.domainStats = function () { return lib.domainStats(h); };
    // energy and momentum diagnostics, reduced on the GPU (fpic_energy_*): scope 'global' (default; collective on a rank
    // with a communicator) or 'local' (this rank's particles and planes)
    const scopeOf = (scope) => (scope === 'local' ? 0 : 1);
    out.energy = function (scope) { return lib.energy(h, scopeOf(scope)); };
    out.recordEnergy = function (every, capacity) { lib.recordEnergy(h, every, capacity === undefined ? 4096 : capacity); };  // every 0: off
    out.energyHistory = function (scope) { return lib.energyHistory(h, scopeOf(scope)); };  // { rows (oldest first), dropped }
    // phase-space histogram of one species, reduced on the GPU (fpic_histogram): request = { axes: one or two names from
    // x y z vx vy vz v2, bins: one count per axis, range: one [lo, hi] per axis, species (default 0) }, over the stored
    // values (positions as fractions of the box, velocities in units of c)
    // -> { counts: BigUint64Array, row-major [bins[0]][bins[1]], outside }
    const HIST_AXES = { x: 0, y: 1, z: 2, vx: 3, vy: 4, vz: 5, v2: 6 };
    out.histogram = function (request, scope) {
        if (request === null || typeof request !== 'object') throw new TypeError('.request <- expected { axes, bins, range, species }');
        const axes = request.axes, bins = request.bins, range = request.range;
        if (!Array.isArray(axes) || (axes.length !== 1 && axes.length !== 2)) throw new RangeError('.axes <- expected an array of one or two axis names');
        if (!Array.isArray(bins) || bins.length !== axes.length || !bins.every((b) => Number.isInteger(b) && b >= 1 && b <= 0x7fffffff)) throw new RangeError('.bins <- expected one positive integer per axis');
        if (!Array.isArray(range) || range.length !== axes.length || !range.every((r) => Array.isArray(r) && r.length === 2 && r.every((x) => typeof x === 'number'))) throw new RangeError('.range <- expected one [lo, hi] per axis');
        const codes = axes.map((a) => { if (!(a in HIST_AXES)) throw new RangeError('.axis <- must be one of x, y, z, vx, vy, vz, v2'); return HIST_AXES[a]; });
        return lib.histogram(h, request.species || 0, Int32Array.from(codes), Int32Array.from(bins), Float64Array.from(range.flat()), scopeOf(scope));
    };
    // selection (fpic_select): the live particles of one species in a window of phase space, filtered and compacted on the GPU.
    // request = { species (default 0), where: { axis: [lo, hi], ... } with names from x y z vx vy vz v2 over the stored values,
    // null for the infinite side (lo <= q < hi), every: [mod, rem] keeps ids with id % mod === rem, capacity: rows to make room
    // for (default: ask for the count first; 0: the count alone), dtype: 'fp32' | 'fp64' (default the handle's) }
    // -> { ids: Uint32Array, position, velocity: [matched][3], matched } in ascending id; the arrays are null when matched
    // exceeds a given capacity
    out.select = function (request, scope) {
        if (request === null || typeof request !== 'object') throw new TypeError('.request <- expected { species, where, every, capacity }');
        const where = request.where === undefined || request.where === null ? {} : request.where;
        if (typeof where !== 'object' || Array.isArray(where)) throw new TypeError('.where <- expected { axis: [lo, hi], ... }');
        const codes = [], ranges = [];
        for (const [name, r] of Object.entries(where)) {
            if (!(name in HIST_AXES)) throw new RangeError('.axis <- must be one of x, y, z, vx, vy, vz, v2');
            if (!Array.isArray(r) || r.length !== 2 || !r.every((x) => x === null || x === undefined || typeof x === 'number')) throw new RangeError('.range <- expected one [lo, hi] per axis, null for the infinite side');
            codes.push(HIST_AXES[name]);
            ranges.push(r[0] === null || r[0] === undefined ? -Infinity : r[0], r[1] === null || r[1] === undefined ? Infinity : r[1]);
        }
        const every = request.every === undefined || request.every === null ? [0, 0] : request.every;
        if (!Array.isArray(every) || every.length !== 2 || !every.every((k) => Number.isInteger(k) && k >= 0 && k <= 0xffffffff)) throw new RangeError('.every <- expected [mod, rem] of unsigned 32-bit integers');
        const capacity = request.capacity === undefined || request.capacity === null ? -1 : request.capacity;
        if (!Number.isInteger(capacity) || capacity < -1) throw new RangeError('.capacity <- expected a non-negative integer');
        if (request.dtype !== undefined && request.dtype !== 'fp32' && request.dtype !== 'fp64') throw new RangeError(".dtype <- must be 'fp32' or 'fp64'");
        const f64 = request.dtype === undefined ? fp64 : request.dtype === 'fp64';
        return lib.select(h, request.species || 0, Int32Array.from(codes), Float64Array.from(ranges), every[0], every[1], capacity, f64 ? 1 : 0, scopeOf(scope));
    };
    // absorbing sinks (fpic_remove*): the particles select() would return leave the species, exactly accounted for.  request =
    // { species (default 0), where, every: as select(), outside: true removes the particles that pass `every` and do NOT lie in
    // the window }.  remove -> { applications, scanned, removed, energyFixed, momentumFixed (BigInt, units of 2^-80 c^2 and c:
    // what the species lost), energy (J), momentum (kg m/s), charge (C) }; removeEvery(period, request) -> the operator's index
    // (it runs after every period-th sub-step and waits for one 8-byte count); removeStats(index, scope) -> its totals;
    // clearRemovals() drops every sink; renumber(species) gives the survivors of a thinned species the ids 0 .. n-1 and returns n
    const removeArgs = function (request) {
        if (request === undefined || request === null) request = {};
        if (typeof request !== 'object' || Array.isArray(request)) throw new TypeError('.request <- expected { species, where, every, outside }');
        const where = request.where === undefined || request.where === null ? {} : request.where;
        if (typeof where !== 'object' || Array.isArray(where)) throw new TypeError('.where <- expected { axis: [lo, hi], ... }');
        const codes = [], ranges = [];
        for (const [name, r] of Object.entries(where)) {
            if (!(name in HIST_AXES)) throw new RangeError('.axis <- must be one of x, y, z, vx, vy, vz, v2');
            if (!Array.isArray(r) || r.length !== 2 || !r.every((x) => x === null || x === undefined || typeof x === 'number')) throw new RangeError('.range <- expected one [lo, hi] per axis, null for the infinite side');
            codes.push(HIST_AXES[name]);
            ranges.push(r[0] === null || r[0] === undefined ? -Infinity : r[0], r[1] === null || r[1] === undefined ? Infinity : r[1]);
        }
        const every = request.every === undefined || request.every === null ? [0, 0] : request.every;
        if (!Array.isArray(every) || every.length !== 2 || !every.every((k) => Number.isInteger(k) && k >= 0 && k <= 0xffffffff)) throw new RangeError('.every <- expected [mod, rem] of unsigned 32-bit integers');
        if (request.outside !== undefined && typeof request.outside !== 'boolean') throw new TypeError('.outside <- must be true or false');
        return [request.species || 0, Int32Array.from(codes), Float64Array.from(ranges), every[0], every[1], request.outside ? 1 : 0];
    };
    out.remove = function (request) {
        const a = removeArgs(request);
        return lib.remove(h, a[0], a[1], a[2], a[3], a[4], a[5]);
    };
    out.removeEvery = function (period, request) {
        if (!Number.isInteger(period)) throw new RangeError('.every <- must be an integer');
        const a = removeArgs(request);
        return lib.removeEvery(h, a[0], a[1], a[2], a[3], a[4], a[5], period);
    };
    out.removeStats = function (index, scope) {
        if (!Number.isInteger(index)) throw new RangeError('.index <- must be an integer');
        return lib.removeStats(h, index, scopeOf(scope));
    };
    out.clearRemovals = function () { lib.clearRemovals(h); };
    out.renumber = function (species) {
        const sp = species || 0, n = lib.renumber(h, sp);
        counts[sp] = n;      // (getParticles and set size their arrays by it)
        return n;
    };
    // particle sources (fpic_reserve, fpic_population, fpic_inject*): a species gains particles generated on the GPU by load()'s
    // rule.  request = load()'s keys (species, count: the particles per application, first: the sequence number of application
    // 0, seed, stream, lo, hi, drift, vth, lattice, paired, mode, xamp, xphase, vamp, vphase) and kind: 'volume' (default) |
    // 'flux', axis (0 .. 2), side (+1 | -1), plane (metres), epoch (applications made before: a resumed registration).
    // inject -> { applications, injected, energyFixed, momentumFixed (BigInt, units of 2^-80 c^2 and c: what the species gained),
    // energy (J), momentum (kg m/s), charge (C) }; injectEvery(period, request) -> the source's index (it runs after every
    // period-th sub-step, after the sinks); injectStats(index, scope) -> its totals; clearInjections() drops every source;
    // reserve(species, capacity) makes the room and returns the capacity; population(species) -> { n, capacity, id_span }
    // (a registered source changes n behind the host: getParticles, getCells and set ask for it themselves)
    const injectArgs = function (request) {
        if (request === null || typeof request !== 'object' || Array.isArray(request)) throw new TypeError('.request <- expected { kind, species, count, first, seed, ... }');
        const kind = request.kind === undefined || request.kind === 'volume' ? 0 : request.kind === 'flux' ? 1 : -1;
        if (kind < 0) throw new RangeError(".kind <- must be 'volume' or 'flux'");
        if (!Number.isInteger(request.count) || request.count < 0) throw new RangeError('.count <- expected the particles per application, a non-negative integer');
        const int32 = function (name, v) {
            if (v === undefined || v === null) v = 0;
            if (!Number.isInteger(v) || v < -0x80000000 || v > 0x7fffffff) throw new RangeError('.' + name + ' <- expected a 32-bit integer');
            return v;
        };
        const plane = request.plane === undefined || request.plane === null ? 0 : request.plane;
        if (typeof plane !== 'number') throw new RangeError('.plane <- expected a number');
        let epoch = request.epoch === undefined || request.epoch === null ? 0n : request.epoch;
        if (typeof epoch === 'number' && Number.isInteger(epoch) && epoch >= 0) epoch = BigInt(epoch);
        if (typeof epoch !== 'bigint' || epoch < 0n || epoch >= (1n << 64n)) throw new RangeError('.epoch <- expected a non-negative integer, or a BigInt up to 2^64');
        const la = loadArgs(Object.assign({}, request, { position: true, velocity: true, append: false }));
        return [la.species, Float64Array.from(la.words), Float64Array.from(la.reals), Float64Array.from([kind, int32('axis', request.axis), int32('side', request.side), plane, Number(epoch & 0xffffffffn), Number(epoch >> 32n)])];
    };
    out.inject = function (request) {
        const a = injectArgs(request), r = lib.inject(h, a[0], a[1], a[2], a[3]);
        live(a[0]);
        return r;
    };
    out.injectEvery = function (period, request) {
        if (!Number.isInteger(period)) throw new RangeError('.every <- must be an integer');
        const a = injectArgs(request);
        return lib.injectEvery(h, a[0], a[1], a[2], a[3], period);
    };
    out.injectStats = function (index, scope) {
        if (!Number.isInteger(index)) throw new RangeError('.index <- must be an integer');
        return lib.injectStats(h, index, scopeOf(scope));
    };
    out.clearInjections = function () { lib.clearInjections(h); };
    out.reserve = function (species, capacity) {
        if (!Number.isInteger(capacity) || capacity < 0) throw new RangeError('.capacity <- expected a non-negative integer');
        return lib.reserve(h, species || 0, capacity);
    };
    out.population = function (species) {
        const sp = species || 0, p = lib.population(h, sp);
        if (!decomposed) counts[sp] = p.n;
        return p;
    };
    // the loader's request as the addon takes it: { species, words, reals, three, whole, real } (load, inject)
    const loadArgs = function (request) {
        if (request === null || typeof request !== 'object') throw new TypeError('.request <- expected { species, first, count, seed, ... }');
        const three = function (name, v, dflt) {
            if (v === undefined || v === null) v = dflt;
            if (typeof v === 'number') v = [v, v, v];
            if (!(Array.isArray(v) || ArrayBuffer.isView(v)) || v.length !== 3 || !Array.from(v).every((x) => typeof x === 'number')) throw new RangeError('.' + name + ' <- expected a number or three of them');
            return Array.from(v);
        };
        const whole = function (name, v, dflt, least, most) {
            if (v === undefined || v === null) v = dflt;
            if (!Number.isInteger(v) || v < least || v > most) throw new RangeError('.' + name + ' <- expected an integer within its field');
            return v;
        };
        const real = function (name, v) {
            if (v === undefined || v === null) v = 0;
            if (typeof v !== 'number') throw new RangeError('.' + name + ' <- expected a number');
            return v;
        };
        let seed = request.seed === undefined || request.seed === null ? 0x5EEDF051 : request.seed;
        if (typeof seed === 'number') {
            if (!Number.isInteger(seed) || seed < 0 || seed > Number.MAX_SAFE_INTEGER) throw new RangeError('.seed <- expected an integer up to 2^53, or a BigInt up to 2^64');
            seed = BigInt(seed);
        }
        if (typeof seed !== 'bigint' || seed < 0n || seed >= (1n << 64n)) throw new RangeError('.seed <- expected an integer up to 2^53, or a BigInt up to 2^64');
        const flags = (request.position === false ? 0 : 1) | (request.velocity === false ? 0 : 2) | (request.lattice ? 4 : 0) | (request.paired ? 8 : 0) | (request.append ? 16 : 0);
        const mode = three('mode', request.mode, 0).map((m) => whole('mode', m, 0, -0x80000000, 0x7fffffff));
        const words = [whole('first', request.first, 0, 0, Number.MAX_SAFE_INTEGER), whole('count', request.count, -1, -1, Number.MAX_SAFE_INTEGER),
            Number(seed & 0xffffffffn), Number(seed >> 32n), whole('stream', request.stream, 0, 0, 0xffffffff), flags].concat(mode);
        const reals = [].concat(three('lo', request.lo, 0), three('hi', request.hi, [spec.radius, spec.length_y, spec.height]), three('drift', request.drift, 0),
            three('vth', request.vth, 0), three('xamp', request.xamp, 0), [real('xphase', request.xphase)], three('vamp', request.vamp, 0), [real('vphase', request.vphase)]);
        const species = whole('species', request.species, 0, 0, 0x7fffffff);
        return { species: species, words: words, reals: reals, three: three, whole: whole, real: real };
    };
    // the loader (fpic_load): particles [first, first + count) of one species generated on the GPU.  request = { species, first,
    // count (default: to the end), seed (an integer up to 2^53 or a BigInt up to 2^64), stream, lo, hi (metres; default the whole
    // box), drift, vth (units of c), mode (three integers), xamp (metres), xphase, vamp (c), vphase (turns), lattice, paired,
    // position, velocity (default true), append, density, thermal, shear (tabulated profiles along the axes: below) }; a number
    // where three are expected is taken for all three -> the particles written (kept, on a rank of a decomposition)
    out.load = function (request) {
        const la = loadArgs(request), species = la.species, words = la.words, reals = la.reals, three = la.three, whole = la.whole, real = la.real;
        // profiles (fpic_load_profile): density, thermal = [x, y, z], each null or a table (an array of numbers or a typed array:
        // 2 .. 1025 nodes over [lo, hi] on its axis, linear between them); shear = { axis, component, values }.  Without any
        // of the three keys the call is fpic_load itself.
        const none = (v) => v === undefined || v === null;
        // a radial body (fpic_load_radial): radial = { geometry: 'sphere' | 'cylinder', center: [x, y, z], r_max, axis (the
        // cylinder's, default 0), density, thermal, flow_radial, flow_azimuthal, flow_axial (tables of 2 .. 1025 nodes over
        // [0, r_max]) }; it does not combine with density, thermal or shear
        if (!none(request.radial)) {
            const rd = request.radial;
            if (typeof rd !== 'object' || Array.isArray(rd)) throw new TypeError('.radial <- expected { geometry, center, r_max, ... }');
            if (!none(request.density) || !none(request.thermal) || !none(request.shear)) throw new RangeError('.radial <- does not combine with density, thermal or shear');
            const geometry = rd.geometry === 'sphere' ? 1 : rd.geometry === 'cylinder' ? 2 : rd.geometry;
            const head = [whole('geometry', geometry, 0, 0, 0xffffffff), whole('axis', rd.axis, 0, -0x80000000, 0x7fffffff)].concat(three('center', rd.center, null), [real('r_max', rd.r_max)]);
            const counts = [], values = [];
            for (const name of ['density', 'thermal', 'flow_radial', 'flow_azimuthal', 'flow_axial']) {
                const v = rd[name];
                if (none(v)) { counts.push(0); continue; }
                if (!(Array.isArray(v) || ArrayBuffer.isView(v)) || !Array.from(v).every((x) => typeof x === 'number')) throw new RangeError('.' + name + ' <- a table must be an array of numbers');
                counts.push(v.length);
                for (const x of v) values.push(x);
            }
            return lib.load(h, species, Float64Array.from(words), Float64Array.from(reals), Float64Array.from(head.concat(counts)), Float64Array.from(values));
        }
        if (none(request.density) && none(request.thermal) && none(request.shear)) return lib.load(h, species, Float64Array.from(words), Float64Array.from(reals));
        const shape = [], tables = [];
        const table = function (name, v) {
            if (!(Array.isArray(v) || ArrayBuffer.isView(v)) || !Array.from(v).every((x) => typeof x === 'number')) throw new RangeError('.' + name + ' <- a table must be an array of numbers');
            shape.push(v.length);
            for (const x of v) tables.push(x);
        };
        for (const name of ['density', 'thermal']) {
            const v = request[name];
            if (none(v)) { shape.push(0, 0, 0); continue; }
            if (!Array.isArray(v) || v.length !== 3) throw new RangeError('.' + name + ' <- expected three entries (x, y, z), each null or a table');
            for (const t of v) { if (none(t)) shape.push(0); else table(name, t); }
        }
        if (none(request.shear)) shape.push(0, 0, 0);
        else {
            const sh = request.shear;
            if (typeof sh !== 'object' || Array.isArray(sh)) throw new TypeError('.shear <- expected { axis, component, values }');
            table('shear', sh.values);
            shape.push(whole('shear_axis', sh.axis, 0, -0x80000000, 0x7fffffff), whole('shear_component', sh.component, 0, -0x80000000, 0x7fffffff));
        }
        return lib.load(h, species, Float64Array.from(words), Float64Array.from(reals), Float64Array.from(shape), Float64Array.from(tables));
    };
    // Monte Carlo collisions with a prescribed drifting Maxwellian (fpic_collide*).  request = { kind: 'exchange' | 'elastic' |
    // 'relax', species, either nu (1/s), sigmaN (density times cross-section, 1/m), tau (s; default the sub-step dt, every * dt
    // for collideEvery) or the dimensionless nuTau, sigmaTau; gMax (c), drift, vth (c; a number is taken for all three),
    // massRatio (default Infinity for 'elastic'), seed (an integer up to 2^53 or a BigInt up to 2^64), stream, epoch }
    // collide -> { applications, candidates, collided, clipped }; collideEvery(every, request) -> the operator's index;
    // collisionStats(index, scope) -> its totals since registration; clearCollisions() drops every operator
    const COLLIDE_KINDS = { exchange: 0, elastic: 1, relax: 2 };
    const collideArgs = function (request, tauDefault) {
        if (request === null || typeof request !== 'object') throw new TypeError('.request <- expected { kind, species, nu, sigmaN, tau, ... }');
        const three = function (name, v) {
            if (v === undefined || v === null) v = 0;
            if (typeof v === 'number') v = [v, v, v];
            if (!(Array.isArray(v) || ArrayBuffer.isView(v)) || v.length !== 3 || !Array.from(v).every((x) => typeof x === 'number')) throw new RangeError('.' + name + ' <- expected a number or three of them');
            return Array.from(v);
        };
        const whole = function (name, v, dflt, least, most) {
            if (v === undefined || v === null) v = dflt;
            if (!Number.isInteger(v) || v < least || v > most) throw new RangeError('.' + name + ' <- expected an integer within its field');
            return v;
        };
        const real = function (name, v, dflt) {
            if (v === undefined || v === null) v = dflt;
            if (typeof v !== 'number') throw new RangeError('.' + name + ' <- expected a number');
            return v;
        };
        const given = (v) => v !== undefined && v !== null;
        let kind = request.kind;
        if (typeof kind === 'string') {
            if (!(kind in COLLIDE_KINDS)) throw new RangeError(".kind <- must be one of 'exchange', 'elastic', 'relax'");
            kind = COLLIDE_KINDS[kind];
        }
        kind = whole('kind', kind, undefined, -0x80000000, 0x7fffffff);
        let seed = given(request.seed) ? request.seed : 0xC0111DE5;
        if (typeof seed === 'number') {
            if (!Number.isInteger(seed) || seed < 0 || seed > Number.MAX_SAFE_INTEGER) throw new RangeError('.seed <- expected an integer up to 2^53, or a BigInt up to 2^64');
            seed = BigInt(seed);
        }
        if (typeof seed !== 'bigint' || seed < 0n || seed >= (1n << 64n)) throw new RangeError('.seed <- expected an integer up to 2^53, or a BigInt up to 2^64');
        const physical = given(request.nu) || given(request.sigmaN) || given(request.tau), pair = given(request.nuTau) || given(request.sigmaTau);
        if (physical && pair) throw new RangeError('.nuTau <- give either nu, sigmaN, tau or nuTau, sigmaTau, not both');
        let nuTau, sigmaTau;
        if (physical) {
            const tau = real('tau', request.tau, tauDefault);
            nuTau = real('nu', request.nu, 0) * tau;
            sigmaTau = real('sigmaN', request.sigmaN, 0) * 2.998e8 * tau;
        } else {
            nuTau = real('nuTau', request.nuTau, 0);
            sigmaTau = real('sigmaTau', request.sigmaTau, 0);
        }
        const words = [kind, Number(seed & 0xffffffffn), Number(seed >> 32n), whole('stream', request.stream, 0, 0, 0xffffffff), whole('epoch', request.epoch, 0, 0, 0xffffffff)];
        const reals = [nuTau, sigmaTau, real('gMax', request.gMax, 0)].concat(three('drift', request.drift), three('vth', request.vth),
            [real('massRatio', request.massRatio, kind === 1 ? Infinity : 0)]);
        return [whole('species', request.species, 0, 0, 0x7fffffff), Float64Array.from(words), Float64Array.from(reals)];
    };
    out.collide = function (request) {
        const a = collideArgs(request, spec.dt);
        return lib.collide(h, a[0], a[1], a[2]);
    };
    out.collideEvery = function (every, request) {
        if (!Number.isInteger(every) || every < -0x80000000 || every > 0x7fffffff) throw new RangeError('.every <- expected a 32-bit integer');
        const a = collideArgs(request, every * spec.dt);
        return lib.collideEvery(h, a[0], a[1], a[2], every);
    };
    out.collisionStats = function (index, scope) {
        if (!Number.isInteger(index) || index < -0x80000000 || index > 0x7fffffff) throw new RangeError('.index <- expected a 32-bit integer');
        return lib.collisionStats(h, index, scopeOf(scope));
    };
    out.clearCollisions = function () { lib.clearCollisions(h); };
    // prescribed external forces (fpic_force*).  request = { waves: [{ amp (V/m or m/s^2; a number is taken for all three),
    // mode: [mx, my, mz], frequency (Hz) | nu (turns per sub-step), phase (turns) }] (1 .. 4), species, kind: 'field' |
    // 'accel', lo, hi (the window in metres; default the whole box), taper: [x, y, z] (each null or the nodes of a table over
    // the window), envelope: { start, stop, values } (active for start <= s <= stop, s = sub-steps since create + epoch;
    // integers up to 2^53 or BigInts up to 2^64), epoch }.  force -> { applications, kicked, workFixed, impulseFixed (BigInt:
    // the exact sums, units of 2^-80 c^2 and c), work (J), impulse (kg m/s) }; forceOn(request) -> the request's index;
    // forceStats(index, scope) -> its totals since registration; clearForces() drops every request
    const FORCE_KINDS = { field: 0, accel: 1 };
    const forceArgs = function (request) {
        if (request === null || typeof request !== 'object' || Array.isArray(request)) throw new TypeError('.request <- expected { waves, species, kind, lo, hi, taper, envelope, epoch }');
        const given = (v) => v !== undefined && v !== null;
        const three = function (name, v, dflt) {
            if (!given(v)) v = dflt;
            if (typeof v === 'number') v = [v, v, v];
            if (!(Array.isArray(v) || ArrayBuffer.isView(v)) || v.length !== 3 || !Array.from(v).every((x) => typeof x === 'number')) throw new RangeError('.' + name + ' <- expected a number or three of them');
            return Array.from(v);
        };
        const whole = function (name, v, dflt, least, most) {
            if (!given(v)) v = dflt;
            if (!Number.isInteger(v) || v < least || v > most) throw new RangeError('.' + name + ' <- expected an integer within its field');
            return v;
        };
        const real = function (name, v, dflt) {
            if (!given(v)) v = dflt;
            if (typeof v !== 'number') throw new RangeError('.' + name + ' <- expected a number');
            return v;
        };
        const wide = function (name, v, dflt) {
            if (!given(v)) v = dflt;
            if (typeof v === 'number') {
                if (!Number.isInteger(v) || v < 0 || v > Number.MAX_SAFE_INTEGER) throw new RangeError('.' + name + ' <- expected an integer up to 2^53, or a BigInt up to 2^64');
                v = BigInt(v);
            }
            if (typeof v !== 'bigint' || v < 0n || v >= (1n << 64n)) throw new RangeError('.' + name + ' <- expected an integer up to 2^53, or a BigInt up to 2^64');
            return [Number(v & 0xffffffffn), Number(v >> 32n)];
        };
        let kind = given(request.kind) ? request.kind : 'field';
        if (typeof kind === 'string') {
            if (!(kind in FORCE_KINDS)) throw new RangeError(".kind <- must be one of 'field', 'accel'");
            kind = FORCE_KINDS[kind];
        }
        kind = whole('kind', kind, undefined, -0x80000000, 0x7fffffff);
        const waves = request.waves;
        if (!Array.isArray(waves)) throw new TypeError('.waves <- expected a list of 1 .. 4 waves');
        const modes = new Array(12).fill(0), wreals = new Array(20).fill(0);
        waves.slice(0, 4).forEach(function (w, k) {
            if (w === null || typeof w !== 'object' || !given(w.amp)) throw new TypeError('.waves <- a wave is { amp, mode, nu | frequency, phase }');
            if (given(w.nu) && given(w.frequency)) throw new RangeError('.nu <- give either nu or frequency, not both');
            const amp = three('amp', w.amp, 0), mode = given(w.mode) ? w.mode : [0, 0, 0];
            if (!Array.isArray(mode) || mode.length !== 3) throw new RangeError('.mode <- expected three integers');
            for (let a = 0; a < 3; ++a) { modes[3 * k + a] = whole('mode', mode[a], 0, -0x80000000, 0x7fffffff); wreals[5 * k + a] = amp[a]; }
            wreals[5 * k + 3] = given(w.frequency) ? real('frequency', w.frequency, 0) * spec.dt : real('nu', w.nu, 0);
            wreals[5 * k + 4] = real('phase', w.phase, 0);
        });
        const box = [spec.radius, spec.length_y, spec.height].map((v) => (typeof v === 'number' ? v : 1));
        const counts = [], tables = [];
        const table = function (name, t) {
            if (!given(t)) { counts.push(0); return; }
            if (!(Array.isArray(t) || ArrayBuffer.isView(t)) || !Array.from(t).every((x) => typeof x === 'number')) throw new RangeError('.' + name + ' <- a table must be a list of numbers');
            counts.push(t.length);
            for (const x of t) tables.push(x);
        };
        const taper = given(request.taper) ? request.taper : [null, null, null];
        if (!Array.isArray(taper) || taper.length !== 3) throw new RangeError('.taper <- expected three entries (x, y, z), each null or a table');
        for (const t of taper) table('taper', t);
        const env = given(request.envelope) ? request.envelope : {};
        if (typeof env !== 'object' || Array.isArray(env)) throw new TypeError('.envelope <- expected { start, stop, values }');
        table('envelope', env.values);
        const words = [kind, waves.length].concat(wide('epoch', request.epoch, 0), wide('start', env.start, 0), wide('stop', env.stop, (1n << 64n) - 1n), modes, counts);
        const reals = three('lo', request.lo, 0).concat(three('hi', request.hi, box), wreals);
        return [whole('species', request.species, 0, 0, 0x7fffffff), Float64Array.from(words), Float64Array.from(reals), Float64Array.from(tables)];
    };
    out.force = function (request) {
        const a = forceArgs(request);
        return lib.force(h, a[0], a[1], a[2], a[3]);
    };
    out.forceOn = function (request) {
        const a = forceArgs(request);
        return lib.forceOn(h, a[0], a[1], a[2], a[3]);
    };
    out.forceStats = function (index, scope) {
        if (!Number.isInteger(index) || index < -0x80000000 || index > 0x7fffffff) throw new RangeError('.index <- expected a 32-bit integer');
        return lib.forceStats(h, index, scopeOf(scope));
    };
    out.clearForces = function () { lib.clearForces(h); };
    // windowed background collisions with a tabulated cross-section (fpic_gas*).  request = { kind: 'exchange' | 'elastic',
    // species, density (m^-3, the peak), tau (s; default the sub-step dt, every * dt for collideGasEvery), sigma (the
    // cross-sections in m^2, 2 .. 4096 of them), gLo, gHi (their first and last relative speed, units of c), drift, vth,
    // massRatio (the background, as collide), lo, hi (the window in metres; default the whole box), taper: [x, y, z] (each
    // null or the nodes in [0, 1] of the density profile over the window), seed, stream, epoch }.  collideGas ->
    // { applications, candidates, collided, below, above, energyFixed, momentumFixed (BigInt: the exact sums of what the
    // species gained, units of 2^-80 c^2 and c), energy (J), momentum (kg m/s) }; collideGasEvery(every, request) -> the
    // operator's index; gasStats(index, scope) -> its totals since registration; clearGas() drops every such operator
    const GAS_KINDS = { exchange: 0, elastic: 1 };
    const gasArgs = function (request, tauDefault) {
        if (request === null || typeof request !== 'object' || Array.isArray(request)) throw new TypeError('.request <- expected { kind, species, density, tau, sigma, gLo, gHi, drift, vth, massRatio, lo, hi, taper, seed, stream, epoch }');
        const given = (v) => v !== undefined && v !== null;
        const three = function (name, v, dflt) {
            if (!given(v)) v = dflt;
            if (typeof v === 'number') v = [v, v, v];
            if (!(Array.isArray(v) || ArrayBuffer.isView(v)) || v.length !== 3 || !Array.from(v).every((x) => typeof x === 'number')) throw new RangeError('.' + name + ' <- expected a number or three of them');
            return Array.from(v);
        };
        const whole = function (name, v, dflt, least, most) {
            if (!given(v)) v = dflt;
            if (!Number.isInteger(v) || v < least || v > most) throw new RangeError('.' + name + ' <- expected an integer within its field');
            return v;
        };
        const real = function (name, v, dflt) {
            if (!given(v)) v = dflt;
            if (typeof v !== 'number') throw new RangeError('.' + name + ' <- expected a number');
            return v;
        };
        let kind = request.kind;
        if (typeof kind === 'string') {
            if (!(kind in GAS_KINDS)) throw new RangeError(".kind <- must be one of 'exchange', 'elastic'");
            kind = GAS_KINDS[kind];
        }
        kind = whole('kind', kind, undefined, -0x80000000, 0x7fffffff);
        let seed = given(request.seed) ? request.seed : 0x6A5C0111DE;
        if (typeof seed === 'number') {
            if (!Number.isInteger(seed) || seed < 0 || seed > Number.MAX_SAFE_INTEGER) throw new RangeError('.seed <- expected an integer up to 2^53, or a BigInt up to 2^64');
            seed = BigInt(seed);
        }
        if (typeof seed !== 'bigint' || seed < 0n || seed >= (1n << 64n)) throw new RangeError('.seed <- expected an integer up to 2^53, or a BigInt up to 2^64');
        const box = [spec.radius, spec.length_y, spec.height].map((v) => (typeof v === 'number' ? v : 1));
        const counts = [], tables = [];
        const table = function (name, t, needed) {
            if (!given(t) && !needed) { counts.push(0); return; }
            if (!(Array.isArray(t) || ArrayBuffer.isView(t)) || t.length > 0x7fffffff || !Array.from(t).every((x) => typeof x === 'number')) throw new RangeError('.' + name + ' <- a table must be a list of numbers');
            counts.push(t.length);
            for (const x of t) tables.push(x);
        };
        table('sigma', request.sigma, true);
        const taper = given(request.taper) ? request.taper : [null, null, null];
        if (!Array.isArray(taper) || taper.length !== 3) throw new RangeError('.taper <- expected three entries (x, y, z), each null or a table');
        for (const t of taper) table('taper', t, false);
        const words = [kind, Number(seed & 0xffffffffn), Number(seed >> 32n), whole('stream', request.stream, 0, 0, 0xffffffff), whole('epoch', request.epoch, 0, 0, 0xffffffff)].concat(counts);
        const reals = [real('density', request.density, undefined), real('tau', request.tau, tauDefault), real('gLo', request.gLo, undefined), real('gHi', request.gHi, undefined)].concat(
            three('drift', request.drift, 0), three('vth', request.vth, 0), [real('massRatio', request.massRatio, kind === 1 ? Infinity : 0)], three('lo', request.lo, 0), three('hi', request.hi, box));
        return [whole('species', request.species, 0, 0, 0x7fffffff), Float64Array.from(words), Float64Array.from(reals), Float64Array.from(tables)];
    };
    out.collideGas = function (request) {
        const a = gasArgs(request, spec.dt);
        return lib.collideGas(h, a[0], a[1], a[2], a[3]);
    };
    out.collideGasEvery = function (every, request) {
        if (!Number.isInteger(every) || every < -0x80000000 || every > 0x7fffffff) throw new RangeError('.every <- expected a 32-bit integer');
        const a = gasArgs(request, every * spec.dt);
        return lib.collideGasEvery(h, a[0], a[1], a[2], a[3], every);
    };
    out.gasStats = function (index, scope) {
        if (!Number.isInteger(index) || index < -0x80000000 || index > 0x7fffffff) throw new RangeError('.index <- expected a 32-bit integer');
        return lib.gasStats(h, index, scopeOf(scope));
    };
    out.clearGas = function () { lib.clearGas(h); };
    // electron-impact ionisation of a background gas (fpic_ionize*).  request = collideGas's without kind and massRatio, plus
    // { species (the projectile), electron (default: species), ion, gThreshold (units of c; gLo >= gThreshold) }.  ionize ->
    // { applications, candidates, below, above, ionised, primary, electron, ion }, each group { energyFixed, momentumFixed
    // (BigInt, units of 2^-80 c^2 and c: what the species gained), energy (J), momentum (kg m/s), charge (C) };
    // ionizeEvery(every, request) -> the ioniser's index (it runs after the sources, before the burners); ionizeStats(index, scope) -> its
    // totals; clearIonization() drops every ioniser.  The targets need the room: reserve() first
    const ionizeArgs = function (request, tauDefault) {
        if (request === null || typeof request !== 'object' || Array.isArray(request)) throw new TypeError('.request <- expected { species, electron, ion, gThreshold, density, tau, sigma, gLo, gHi, drift, vth, lo, hi, taper, seed, stream, epoch }');
        const given = (v) => v !== undefined && v !== null;
        const a = gasArgs(Object.assign({}, request, { kind: 0, massRatio: 0, seed: given(request.seed) ? request.seed : 0x1051E0C0FFEE }), tauDefault);
        const target = function (name, v) {
            if (!Number.isInteger(v) || v < -0x80000000 || v > 0x7fffffff) throw new RangeError('.' + name + ' <- expected an integer within its field');
            return v;
        };
        if (typeof request.gThreshold !== 'number') throw new RangeError('.gThreshold <- expected a number');
        a.push(Float64Array.from([target('electron', given(request.electron) ? request.electron : a[0]), target('ion', request.ion), request.gThreshold]));
        return a;
    };
    out.ionize = function (request) {
        const a = ionizeArgs(request, spec.dt), r = lib.ionize(h, a[0], a[1], a[2], a[3], a[4]);
        live(a[0]); live(a[4][0]); live(a[4][1]);
        return r;
    };
    out.ionizeEvery = function (every, request) {
        if (!Number.isInteger(every) || every < -0x80000000 || every > 0x7fffffff) throw new RangeError('.every <- expected a 32-bit integer');
        const a = ionizeArgs(request, every * spec.dt);
        return lib.ionizeEvery(h, a[0], a[1], a[2], a[3], a[4], every);
    };
    out.ionizeStats = function (index, scope) {
        if (!Number.isInteger(index) || index < -0x80000000 || index > 0x7fffffff) throw new RangeError('.index <- expected a 32-bit integer');
        return lib.ionizeStats(h, index, scopeOf(scope));
    };
    out.clearIonization = function () { lib.clearIonization(h); };
    // binary Coulomb collisions between the species of the box (Takizuka-Abe; fpic_pair*).  request = { a, b (default a: like
    // particles), logLambda, tau (s; default the sub-step dt, every * dt for collidePairEvery), seed (an integer up to 2^53 or a
    // BigInt up to 2^64), stream, epoch }.  collidePair -> { applications, pairs, strong, cells, overfullCells,
    // overfullParticles }; collidePairEvery(every, request) -> the operator's index; pairStats(index, scope) -> its totals
    // since registration; clearPairs() drops every pair operator (those of collideEvery stay)
    const pairArgs = function (request, tauDefault) {
        if (request === null || typeof request !== 'object') throw new TypeError('.request <- expected { a, b, logLambda, tau, ... }');
        const whole = function (name, v, dflt, least, most) {
            if (v === undefined || v === null) v = dflt;
            if (!Number.isInteger(v) || v < least || v > most) throw new RangeError('.' + name + ' <- expected an integer within its field');
            return v;
        };
        const real = function (name, v, dflt) {
            if (v === undefined || v === null) v = dflt;
            if (typeof v !== 'number') throw new RangeError('.' + name + ' <- expected a number');
            return v;
        };
        const given = (v) => v !== undefined && v !== null;
        let seed = given(request.seed) ? request.seed : 0x7A1C12ABE;
        if (typeof seed === 'number') {
            if (!Number.isInteger(seed) || seed < 0 || seed > Number.MAX_SAFE_INTEGER) throw new RangeError('.seed <- expected an integer up to 2^53, or a BigInt up to 2^64');
            seed = BigInt(seed);
        }
        if (typeof seed !== 'bigint' || seed < 0n || seed >= (1n << 64n)) throw new RangeError('.seed <- expected an integer up to 2^53, or a BigInt up to 2^64');
        const a = whole('a', request.a, 0, -0x80000000, 0x7fffffff);
        const words = [a, whole('b', request.b, a, -0x80000000, 0x7fffffff), Number(seed & 0xffffffffn), Number(seed >> 32n),
            whole('stream', request.stream, 0, 0, 0xffffffff), whole('epoch', request.epoch, 0, 0, 0xffffffff)];
        return [Float64Array.from(words), Float64Array.from([real('logLambda', request.logLambda, undefined), real('tau', request.tau, tauDefault)])];
    };
    out.collidePair = function (request) {
        const a = pairArgs(request, spec.dt);
        return lib.collidePair(h, a[0], a[1]);
    };
    out.collidePairEvery = function (every, request) {
        if (!Number.isInteger(every) || every < -0x80000000 || every > 0x7fffffff) throw new RangeError('.every <- expected a 32-bit integer');
        const a = pairArgs(request, every * spec.dt);
        return lib.collidePairEvery(h, a[0], a[1], every);
    };
    out.pairStats = function (index, scope) {
        if (!Number.isInteger(index) || index < -0x80000000 || index > 0x7fffffff) throw new RangeError('.index <- expected a 32-bit integer');
        return lib.pairStats(h, index, scopeOf(scope));
    };
    out.clearPairs = function () { lib.clearPairs(h); };
    // fusion yield tallies between the species of the box (fpic_fusion*): a tally, not a sink — no particle changes.
    // request = { a, b (default a: a species with itself), sigma: the table (an array or Float64Array of 2 .. 4096
    // cross-sections in m^2) at relative speeds uniform from gLo to gHi (units of c), tau (s; default the sub-step dt, every * dt
    // for fusionYieldEvery), seed (an integer up to 2^53 or a BigInt up to 2^64), stream, epoch, grid (fusionYield: true adds the
    // cell tallies) }.  fusionYield -> { applications, pairs, below, above, cells, overfullCells, overfullParticles, yieldHi,
    // yieldLo, unitExponent, reactionsExact (a BigInt in units of 2^unitExponent reactions), reactions (a number), grid (a
    // BigInt64Array of nz*ny*nx cells, x fastest, in the same unit) }; fusionYieldEvery(every, request) -> the operator's index;
    // fusionStats(index, scope) -> its totals since registration or the last reset; fusionGrid(index, reset) -> its cell
    // tallies, reset = true zeroes grid, totals and applications behind the copy; clearFusion() drops every tally
    const fusionArgs = function (request, tauDefault) {
        if (request === null || typeof request !== 'object') throw new TypeError('.request <- expected { a, b, sigma, gLo, gHi, tau, ... }');
        const whole = function (name, v, dflt, least, most) {
            if (v === undefined || v === null) v = dflt;
            if (!Number.isInteger(v) || v < least || v > most) throw new RangeError('.' + name + ' <- expected an integer within its field');
            return v;
        };
        const real = function (name, v, dflt) {
            if (v === undefined || v === null) v = dflt;
            if (typeof v !== 'number') throw new RangeError('.' + name + ' <- expected a number');
            return v;
        };
        const given = (v) => v !== undefined && v !== null;
        let seed = given(request.seed) ? request.seed : 0xF0510D7;
        if (typeof seed === 'number') {
            if (!Number.isInteger(seed) || seed < 0 || seed > Number.MAX_SAFE_INTEGER) throw new RangeError('.seed <- expected an integer up to 2^53, or a BigInt up to 2^64');
            seed = BigInt(seed);
        }
        if (typeof seed !== 'bigint' || seed < 0n || seed >= (1n << 64n)) throw new RangeError('.seed <- expected an integer up to 2^53, or a BigInt up to 2^64');
        let sigma = request.sigma;
        if (Array.isArray(sigma)) {
            if (!sigma.every((x) => typeof x === 'number')) throw new TypeError('.sigma <- expected an array of numbers or a Float64Array');
            sigma = Float64Array.from(sigma);
        }
        if (!(sigma instanceof Float64Array)) throw new TypeError('.sigma <- expected an array of numbers or a Float64Array');
        const a = whole('a', request.a, 0, -0x80000000, 0x7fffffff);
        const words = [a, whole('b', request.b, a, -0x80000000, 0x7fffffff), Number(seed & 0xffffffffn), Number(seed >> 32n),
            whole('stream', request.stream, 0, 0, 0xffffffff), whole('epoch', request.epoch, 0, 0, 0xffffffff)];
        return [Float64Array.from(words), Float64Array.from([real('tau', request.tau, tauDefault), real('gLo', request.gLo, undefined), real('gHi', request.gHi, undefined)]), sigma];
    };
    const fusionCounts = function (r) {
        const exact = (BigInt(r.yieldTop) << 64n) + (BigInt(r.yieldMid) << 32n) + BigInt(r.yieldLo);
        r.yieldHi = r.yieldTop * 4294967296 + r.yieldMid;      // (exact below 2^53)
        delete r.yieldTop;
        delete r.yieldMid;
        r.reactionsExact = exact;
        r.reactions = Number(exact) * Math.pow(2, r.unitExponent);
        return r;
    };
    out.fusionYield = function (request) {
        const a = fusionArgs(request, spec.dt);
        const grid = request.grid ? new BigInt64Array(nodes) : null;
        const r = fusionCounts(lib.fusionYield(h, a[0], a[1], a[2], grid));
        if (grid) r.grid = grid;
        return r;
    };
    out.fusionYieldEvery = function (every, request) {
        if (!Number.isInteger(every) || every < -0x80000000 || every > 0x7fffffff) throw new RangeError('.every <- expected a 32-bit integer');
        const a = fusionArgs(request, every * spec.dt);
        return lib.fusionYieldEvery(h, a[0], a[1], a[2], every);
    };
    out.fusionStats = function (index, scope) {
        if (!Number.isInteger(index) || index < -0x80000000 || index > 0x7fffffff) throw new RangeError('.index <- expected a 32-bit integer');
        return fusionCounts(lib.fusionStats(h, index, scopeOf(scope)));
    };
    out.fusionGrid = function (index, reset) {
        if (!Number.isInteger(index) || index < -0x80000000 || index > 0x7fffffff) throw new RangeError('.index <- expected a 32-bit integer');
        const grid = new BigInt64Array(nodes);
        lib.fusionGrid(h, index, grid, reset ? 1 : 0);
        return grid;
    };
    out.clearFusion = function () { lib.clearFusion(h); };
    // fusion burn (fpic_burn*): the pairs of fusionYield react — both reactants leave their species and one new particle each is
    // born in the product species.  request = the request of fusionYield and { products: [p3, p4 or null (the fourth particle
    // leaves the box)], qValue (J), otherMass (kg; with p4 null) }.  burn -> { applications, pairs, below, above, cells,
    // overfullCells, overfullParticles, accepted, blocked, saturated, burnt, reactantA, reactantB (what the species lost),
    // productA, productB (what they gained) }, each group { energyFixed, momentumFixed (BigInt, units of 2^-80 c^2 and c),
    // energy (J), momentum (kg m/s), charge (C) }; burnEvery(every, request) -> the burner's index (it runs after the ionisers);
    // burnStats(index, scope) -> its totals; clearBurn() drops every burner.  The products need the room: reserve() first
    const burnArgs = function (request, tauDefault) {
        if (request === null || typeof request !== 'object' || Array.isArray(request)) throw new TypeError('.request <- expected { a, b, products, sigma, gLo, gHi, tau, qValue, otherMass, seed, stream, epoch }');
        const given = (v) => v !== undefined && v !== null;
        const a = fusionArgs(Object.assign({}, request, { seed: given(request.seed) ? request.seed : 0xB0510C0FFEE }), tauDefault);
        const products = request.products;
        if (!Array.isArray(products) || products.length !== 2) throw new RangeError('.products <- expected [productA, productB or null]');
        const target = function (name, v) {
            if (!Number.isInteger(v) || v < -0x80000000 || v > 0x7fffffff) throw new RangeError('.' + name + ' <- expected an integer within its field');
            return v;
        };
        const real = function (name, v) {
            if (!given(v)) v = 0;
            if (typeof v !== 'number') throw new RangeError('.' + name + ' <- expected a number');
            return v;
        };
        const extra = Float64Array.from([target('productA', products[0]), given(products[1]) ? target('productB', products[1]) : -1, real('qValue', request.qValue), real('otherMass', request.otherMass)]);
        return [a[0], a[1], a[2], extra];
    };
    out.burn = function (request) {
        const a = burnArgs(request, spec.dt), r = lib.burn(h, a[0], a[1], a[2], a[3]);
        live(a[0][0]); live(a[0][1]); live(a[3][0]);
        if (a[3][1] >= 0) live(a[3][1]);
        return r;
    };
    out.burnEvery = function (every, request) {
        if (!Number.isInteger(every) || every < -0x80000000 || every > 0x7fffffff) throw new RangeError('.every <- expected a 32-bit integer');
        const a = burnArgs(request, every * spec.dt);
        return lib.burnEvery(h, a[0], a[1], a[2], a[3], every);
    };
    out.burnStats = function (index, scope) {
        if (!Number.isInteger(index) || index < -0x80000000 || index > 0x7fffffff) throw new RangeError('.index <- expected a 32-bit integer');
        return lib.burnStats(h, index, scopeOf(scope));
    };
    out.clearBurn = function () { lib.clearBurn(h); };
    // fusion product spectra (fpic_fusion_spectrum*): the yield of a fusionYield request distributed over an energy axis.
    // request = the request of fusionYield and { axis: 'product' (default) or 'cm', bins (1 .. 256), lo, hi (J), qValue (J),
    // productMass, otherMass (kg; axis 'product'), los: [x, y, z] (absent or zeros: isotropic emission) }.  fusionSpectrum ->
    // the counts of fusionYield and { edges (Float64Array of bins + 1, J), bins (an array of BigInts in units of
    // 2^unitExponent reactions), under, over (BigInts), yield (Float64Array, reactions) }: the bins, under and over add to
    // reactionsExact.  fusionSpectrumEvery(every, request) -> the operator's index; fusionSpectrumRead(index, reset) -> its
    // totals and words since registration or the last reset, reset = true zeroes them behind the copy; clearFusionSpectra()
    // drops every spectrum
    const spectrumAxes = new Map();
    const spectrumArgs = function (request, tauDefault) {
        const a = fusionArgs(request, tauDefault);
        const real = function (name, v, dflt) {
            if (v === undefined || v === null) v = dflt;
            if (typeof v !== 'number') throw new RangeError('.' + name + ' <- expected a number');
            return v;
        };
        const kind = request.axis === undefined || request.axis === null ? 'product' : request.axis;
        if (kind !== 'product' && kind !== 'cm') throw new RangeError('.axis <- expected \'product\' or \'cm\'');
        if (!Number.isInteger(request.bins) || request.bins < 1 || request.bins > 256) throw new RangeError('.bins <- must be 1 .. FPIC_FUSION_SPECTRUM_BINS_MAX (256)');
        let los = request.los === undefined || request.los === null ? [0, 0, 0] : request.los;
        if (!Array.isArray(los) || los.length !== 3 || !los.every((x) => typeof x === 'number')) throw new TypeError('.los <- expected three numbers');
        const axis = Float64Array.from([kind === 'cm' ? 0 : 1, request.bins, real('lo', request.lo, undefined), real('hi', request.hi, undefined), real('qValue', request.qValue, 0),
            real('productMass', request.productMass, 0), real('otherMass', request.otherMass, 0), los[0], los[1], los[2]]);
        return [a[0], a[1], a[2], axis];
    };
    const spectrumResult = function (r, words, axis) {
        r = fusionCounts(r);
        const bins = axis.bins;
        const entry = (k) => (words[2 * k] << 32n) + words[2 * k + 1];
        r.edges = Float64Array.from({ length: bins + 1 }, (_, k) => axis.lo + (axis.hi - axis.lo) * k / bins);
        r.bins = Array.from({ length: bins }, (_, k) => entry(k));
        r.under = entry(bins);
        r.over = entry(bins + 1);
        r.yield = Float64Array.from(r.bins, (x) => Number(x) * Math.pow(2, r.unitExponent));
        return r;
    };
    out.fusionSpectrum = function (request) {
        const a = spectrumArgs(request, spec.dt);
        const axis = { bins: a[3][1], lo: a[3][2], hi: a[3][3] };
        const words = new BigUint64Array(2 * (axis.bins + 2));
        return spectrumResult(lib.fusionSpectrum(h, a[0], a[1], a[2], a[3], words), words, axis);
    };
    out.fusionSpectrumEvery = function (every, request) {
        if (!Number.isInteger(every) || every < -0x80000000 || every > 0x7fffffff) throw new RangeError('.every <- expected a 32-bit integer');
        const a = spectrumArgs(request, every * spec.dt);
        const index = lib.fusionSpectrumEvery(h, a[0], a[1], a[2], a[3], every);
        spectrumAxes.set(index, { bins: a[3][1], lo: a[3][2], hi: a[3][3] });
        return index;
    };
    out.fusionSpectrumRead = function (index, reset) {
        if (!Number.isInteger(index) || index < -0x80000000 || index > 0x7fffffff) throw new RangeError('.index <- expected a 32-bit integer');
        const axis = spectrumAxes.get(index) || { bins: 256, lo: 0, hi: 1 };      // (an unknown index: the library refuses it)
        const words = new BigUint64Array(2 * (256 + 2));                          // (room for the cap: the addon checks it)
        return spectrumResult(lib.fusionSpectrumRead(h, index, words, reset ? 1 : 0), words, axis);
    };
    out.clearFusionSpectra = function () { lib.clearFusionSpectra(h); spectrumAxes.clear(); };
    // series (fpic_series_*): the field at points and the state of tracer particles as rows of 8 doubles, now or recorded into a
    // device ring.  request = { points: [[x, y, z], ...] in metres (wrapped periodically), tracers: particle indices, species: one
    // index or one per tracer (default 0) }; either list may be missing, not both.  A point row is Ex Ey Ez phi Bx By Bz present,
    // a tracer row x y z vx vy vz found 0 (the stored values).
    const seriesArgs = function (request) {
        if (request === null || typeof request !== 'object') throw new TypeError('.request <- expected { points, tracers, species }');
        const points = request.points === undefined || request.points === null ? [] : request.points;
        const tracers = request.tracers === undefined || request.tracers === null ? [] : Array.from(request.tracers);
        if (!Array.isArray(points) || !points.every((p) => (Array.isArray(p) || ArrayBuffer.isView(p)) && p.length === 3 && Array.from(p).every((x) => typeof x === 'number')))
            throw new RangeError('.points <- expected an array of [x, y, z]');
        if (!tracers.every((t) => Number.isInteger(t) && t >= 0 && t <= 0xffffffff)) throw new RangeError('.tracers <- expected particle indices (uint32)');
        let species = request.species === undefined ? 0 : request.species;
        if (typeof species === 'number') species = tracers.map(() => species);
        else species = Array.from(species);
        if (species.length !== tracers.length || !species.every((x) => Number.isInteger(x) && Math.abs(x) <= 0x7fffffff)) throw new RangeError('.species <- expected one index, or one per tracer');
        return [Float64Array.from(points.map((p) => Array.from(p)).flat()), Int32Array.from(species), Uint32Array.from(tracers)];
    };
    // -> { points: Float64Array [P][8], tracers: Float64Array [M][8] }
    out.series = function (request, scope) { return lib.series(h, ...seriesArgs(request), scopeOf(scope)); };
    // after every `every`-th sub-step the same rows go into a ring of `capacity` rows on the device (every 0: off)
    out.recordSeries = function (every, capacity, request) {
        const args = every ? seriesArgs(request) : [null, null, null];
        lib.recordSeries(h, every, capacity === undefined ? 4096 : capacity, ...args);
    };
    // -> { rows, dropped, substep: Float64Array [rows], points: Float64Array [rows][P][8], tracers: Float64Array [rows][M][8] }, oldest first
    out.seriesHistory = function (scope) { return lib.seriesHistory(h, scopeOf(scope)); };
    // modes (fpic_modes_*): the complex Fourier amplitudes A(m) = (1/N) sum F exp(-2 pi i (mx i / nx + my j / ny + mz k / nz)) of the
    // node fields at chosen wave vectors, summed in double on the GPU, now or recorded into a device ring.  request = { modes:
    // [[mx, my, mz], ...] (integers within [-n/2, n/2] per axis), fields: names from ex ey ez phi bx by bz rho (default the first
    // four) } -> { fields: the selected names in the order of the values, values: Float64Array [M][nq][2] of interleaved re, im }
    const MODE_FIELDS = ['ex', 'ey', 'ez', 'phi', 'bx', 'by', 'bz', 'rho'];
    let recordedModeFields = [];
    const modesArgs = function (request) {
        if (request === null || typeof request !== 'object') throw new TypeError('.request <- expected { modes, fields }');
        const modes = request.modes === undefined || request.modes === null ? [] : request.modes;
        if (!Array.isArray(modes) || !modes.every((m) => (Array.isArray(m) || ArrayBuffer.isView(m)) && m.length === 3 && Array.from(m).every((x) => Number.isInteger(x) && Math.abs(x) <= 0x7fffffff)))
            throw new RangeError('.modes <- expected an array of integer triples [mx, my, mz]');
        const fields = request.fields === undefined ? MODE_FIELDS.slice(0, 4) : request.fields;
        if (!Array.isArray(fields) || !fields.every((f) => MODE_FIELDS.includes(f))) throw new RangeError('.fields <- must be names from ex, ey, ez, phi, bx, by, bz, rho');
        let mask = 0;
        for (const f of fields) mask |= 1 << MODE_FIELDS.indexOf(f);
        return [Int32Array.from(modes.map((m) => Array.from(m)).flat()), mask, MODE_FIELDS.filter((f) => fields.includes(f))];
    };
    out.modes = function (request, scope) {
        const [modes, mask, names] = modesArgs(request);
        return { fields: names, values: lib.modes(h, modes, mask, scopeOf(scope)) };
    };
    // after every `every`-th sub-step the same row goes into a ring of `capacity` rows on the device (every 0: off)
    out.recordModes = function (every, capacity, request) {
        const [modes, mask, names] = every ? modesArgs(request) : [null, 0, []];
        lib.recordModes(h, every, capacity === undefined ? 4096 : capacity, modes, mask);
        recordedModeFields = names;
    };
    // -> { rows, dropped, substep: Float64Array [rows], fields, values: Float64Array [rows][M][nq][2] }, oldest first
    out.modesHistory = function (scope) { return Object.assign(lib.modesHistory(h, scopeOf(scope)), { fields: recordedModeFields }); };
    // fluid moment grids of one species, reduced on the GPU (fpic_moments): request = { species (default 0), which: 'n' | 'order1' |
    // 'order2' (default) | an array of names from N FX FY FZ SXX SYY SZZ SXY SXZ SYZ }
    // -> { NAME: BigInt64Array [nz][ny][nr] per moment asked for (N in units of 2^-42 particles, the others of 2^-32), rejected, spilled }
    const MOMENT_NAMES = ['N', 'FX', 'FY', 'FZ', 'SXX', 'SYY', 'SZZ', 'SXY', 'SXZ', 'SYZ'];
    const MOMENT_SETS = { n: 0x001, order1: 0x00F, order2: 0x3FF };
    out.moments = function (request, scope) {
        if (request === null || typeof request !== 'object') throw new TypeError('.request <- expected { species, which }');
        const which = request.which === undefined ? 'order2' : request.which;
        let mask = 0;
        if (typeof which === 'string') {
            if (!(which in MOMENT_SETS)) throw new RangeError('.which <- must be one of n, order1, order2 or an array of moment names');
            mask = MOMENT_SETS[which];
        } else if (Array.isArray(which)) {
            for (const name of which) {
                const bit = MOMENT_NAMES.indexOf(name);
                if (bit < 0) throw new RangeError('.which <- no such moment: must be among ' + MOMENT_NAMES.join(' '));
                mask |= 1 << bit;
            }
        } else {
            throw new TypeError('.which <- must be one of n, order1, order2 or an array of moment names');
        }
        if (mask === 0) throw new RangeError('.mask <- no moment asked for');
        const names = MOMENT_NAMES.filter((_, b) => (mask >> b) & 1);
        const grids = new BigInt64Array(names.length * nodes);
        const res = lib.moments(h, request.species || 0, mask, scopeOf(scope), grids);
        names.forEach((name, k) => { res[name] = grids.subarray(k * nodes, (k + 1) * nodes); });
        return res;
    };
    out.saveCheckpoint = function (path) { lib.saveCheckpoint(h, String(path)); };   // fpic_save_checkpoint: particles of every species + fields
    out.loadCheckpoint = function (path) { lib.loadCheckpoint(h, String(path)); };
    out.sort = function () { lib.sort(h); };
    out.sync = function () { lib.sync(h); };
    out.profile = function (on) { lib.profile(h, on ? 1 : 0); };
    out.stats = function () { return lib.getStats(h); };
    out.resetStats = function () { lib.resetStats(h); };
    out.destroy = function () { if (h) { lib.destroy(h); h = null; } };
    out.nparticles = n0;
    return addStepAsync(out, lib, () => h);
}

exports.makeCylindricalParticlePusher = function (spec) {
    validate_object(spec, {           // empic.js:31-41
        radius: 'number', height: 'number', nr: 'number', nz: 'number', dt: 'number',
        nparticles: 'number', particle_mass: 'number', particle_charge: 'number',
        precision: [, 'string'], device: [, 'number'], count: [, 'number'], compat: [, 'boolean'],
        sort_interval: [, 'number'], rng: [, 'string'], seed: [, 'number'], geometry: [, 'string'], shape: [, 'string'], raster_subpixel_bits: [, 'number'],
    });
    if (spec.devices !== undefined) {   // SURVEY 8(b) extension key: one process drives one GPU here; N GPUs are N processes (commInit)
        if (!Array.isArray(spec.devices) || spec.devices.length !== 1 || typeof spec.devices[0] !== 'number') {
            throw new Error(".devices <- one process drives one GPU: name one device and start one process per GPU (commUniqueId / commInit)");
        }
        spec = Object.assign({}, spec, { device: spec.devices[0] });
    }
    if (spec.geometry !== undefined && spec.geometry !== 'cyl_rz' && spec.geometry !== 'cart3d') throw new Error(".geometry <- must be 'cyl_rz' or 'cart3d'");
    if (spec.shape !== undefined && spec.shape !== 'ref11' && spec.shape !== 'cic') throw new Error(".shape <- must be 'ref11' or 'cic'");
    if (spec.geometry === 'cart3d') return makeBox(spec, addon());
    // two admissible types: checked by hand, the reference's validator stops at the first alternative
    if (spec.fuse_deposit !== undefined && typeof spec.fuse_deposit !== 'boolean' && spec.fuse_deposit !== 'census') {
        throw new Error(".fuse_deposit <- must be true, false or 'census'");
    }
    const n = spec.count ? spec.count : spec.nparticles * spec.nparticles;   // empic.js:107-109
    const fp64 = spec.precision === 'fp64';
    if (spec.precision !== undefined && spec.precision !== 'fp32' && spec.precision !== 'fp64') {
        throw new Error(".precision <- must be 'fp32' or 'fp64'");
    }
    if (spec.rng !== undefined && spec.rng !== 'reference' && spec.rng !== 'counter') {
        throw new Error(".rng <- must be 'reference' or 'counter'");
    }
    const seed = spec.seed || 0;
    const lib = addon();
    let h = lib.create(spec.radius, spec.height, spec.nr, spec.nz, spec.dt, spec.nparticles, spec.particle_mass,
        spec.particle_charge, spec.count || 0, fp64 ? 1 : 0, spec.device || 0, spec.compat === false ? 1 : 0,
        spec.sort_interval || 0, spec.fuse_deposit === 'census' ? 2 : (spec.fuse_deposit === false ? 1 : 0), spec.rng === 'counter' ? 1 : 0,
        seed % 4294967296, Math.floor(seed / 4294967296) % 4294967296, 0, 0, 0, 0, 0, spec.shape === 'cic' ? 1 : 0, spec.raster_subpixel_bits || 0);
    const nr = spec.nr, nz = spec.nz;
    const Real = fp64 ? Float64Array : Float32Array;
    const out = {};

    out.set = function (value) {                                              // empic.js:1157-1350
        if (value.E) lib.setGrid(h, GRID_IN.E, flattenGrid(value.E, nr, nz, 3, 'E'), nr, nz, 3);
        if (value.B) lib.setGrid(h, GRID_IN.B, flattenGrid(value.B, nr, nz, 3, 'B'), nr, nz, 3);
        if (value.position) lib.setParticles(h, flattenParticles(value.position, n, 'position'), null);
        if (value.velocity) lib.setParticles(h, null, flattenParticles(value.velocity, n, 'velocity'));
        if (value.sink_mask) lib.setGrid(h, GRID_IN.sink_mask, flattenGrid(value.sink_mask, nr, nz, 1, 'sink_mask'), nr, nz, 1);
        if (value.source_pdf) lib.setGrid(h, GRID_IN.source_pdf, flattenGrid(value.source_pdf, nr, nz, 1, 'source_pdf'), nr, nz, 1);
    };
    out.addCurrentLoop = function (r, z, I) { lib.addCurrentLoop(h, r, z, I); };   // empic.js:1352
    out.addCurrentZ = function (I) { lib.addCurrentZ(h, I); };                     // empic.js:1380
    out.addBZ = function (Bz) { lib.addBZ(h, Bz); };                               // empic.js:1391
    out.addBTheta = function (Btheta) { lib.addBTheta(h, Btheta); };               // empic.js:1402
    out.addSpindleCuspPlasmaField = function () {                                 // empic.js:1369
        // the reference's implementation stops at undefined symbols (spindle.js:328, :624, :643)
        throw new Error('addSpindleCuspPlasmaField is not functional in the reference (spindle.js:328)');
    };
    out.precalc = function () { lib.precalc(h); };                                 // empic.js:1413
    out.step = function (ncalls) { lib.step(h, ncalls === undefined ? 1 : ncalls); };  // empic.js:1436
    out.substeps = function (n) { lib.substeps(h, n === undefined ? 1 : n); };         // extension: single sub-steps, step(k) = substeps(2 k)
    out.density = function () { lib.density(h); };                                 // empic.js:1471

    // ---- stand-ins for `canvas` and the reference's unseeded randomness
    out.deposit = function () { lib.deposit(h); };
    out.densityFinish = function () { lib.densityFinish(h); };
    out.readGrid = function (name, buf) {
        if (!(name in GRID_OUT)) throw new Error('.name <- unknown grid ' + name);
        const cells = name === 'inv_cdf' ? 512 * 512 : nr * nz;
        return lib.readGrid(h, GRID_OUT[name], checkLength(buf, 4 * cells, 'out') || new Real(4 * cells));
    };
    out.readDensity = function (buf) { return out.readGrid('avg', buf); };
    out.readMoments = function (buf) { return out.readGrid('moments', buf); };
    out.getParticles = function (into) {
        const r = into || { position: new Real(3 * n), velocity: new Real(3 * n), rand: new Float32Array(4 * n), alive: new Uint8Array(n) };
        checkLength(r.position, 3 * n, 'position'); checkLength(r.velocity, 3 * n, 'velocity');
        checkLength(r.rand, 4 * n, 'rand'); checkLength(r.alive, n, 'alive');
        lib.getParticles(h, r.position || null, r.velocity || null, r.rand || null, r.alive || null);
        return r;
    };
    out.getCells = function (buf) { return lib.getCells(h, checkLength(buf, n, 'cells') || new Int32Array(n)); };
    out.setRandomState = function (state) {
        const f32 = function (a) { return a === undefined || a === null ? null : (a instanceof Float32Array ? a : Float32Array.from(a)); };
        lib.setRandomState(h, checkLength(f32(state.entropy), 4 * 1024 * 1024, 'entropy'), checkLength(f32(state.rand), 4 * n, 'rand'));
    };
    out.commInit = function (id, rank, world, overlap) { lib.commInit(h, id, rank, world, overlap === false ? 0 : 1); };
    out.commDestroy = function () { lib.commDestroy(h); };
    out.commInfo = function () { return lib.commInfo(h); };                  // { rank, world } as the library sees them
    out.saveCheckpoint = function (path) { lib.saveCheckpoint(h, String(path)); };
    out.loadCheckpoint = function (path) { lib.loadCheckpoint(h, String(path)); };
    out.sort = function () { lib.sort(h); };
    out.sync = function () { lib.sync(h); };
    out.profile = function (on) { lib.profile(h, on ? 1 : 0); };
    out.stats = function () { return lib.getStats(h); };
    out.resetStats = function () { lib.resetStats(h); };
    out.destroy = function () { if (h) { lib.destroy(h); h = null; } };
    out.nparticles = n;
    return addStepAsync(out, lib, () => h);
};

exports.validate_object = validate_object;
exports._addon = addon; // shared with matrix_native.js
exports.buildArch = function () { return addon().buildArch(); };
exports.commUniqueId = function () { return addon().commUniqueId(); };   // rank 0; hand the 128 bytes to every rank
