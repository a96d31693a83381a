#!/usr/bin/env node
/*
 * plasma_box_node.js — the self-consistent box (extension, no reference counterpart) from Node: a cold electron
 * plasma against a neutralising background, displaced by a small sinusoidal perturbation, oscillating at the plasma
 * frequency.  Prints the field energy per frame and the frequency measured from its zero crossings beside
 * omega_p * cos(k dx / 2), the dispersion of the scheme (DESIGN.md 4.4).
 *
 *   node examples/plasma_box_node.js [--grid 32] [--perCell 8] [--frames 120] [--solver poisson_fft|yee] [--load]
 *
 * --load makes the cold plasma on the GPU with load() (fpic_load: a Kronecker lattice displaced by the same sine) instead of
 * the loop below; no host arrays are built.  That lattice is not aligned with the grid as the loop's is: its density noise
 * rides on the oscillation and the measured frequency agrees to a few per cent (2.6e-2 at the defaults) instead of 1e-4.
 *
 * Same surface as the reference's pusher (makeCylindricalParticlePusher -> set / precalc / step), selected by the
 * extension key geometry:'cart3d'.
 */
'use strict';
const path = require('path');
const empic = require(path.join(__dirname, '..', 'fusion-sim_amd', 'js', 'empic_native.js'));

const args = { grid: 32, perCell: 8, frames: 120, solver: 'poisson_fft' };
const argv = process.argv.slice(2).filter((a) => a !== '--load');
const useLoad = argv.length !== process.argv.length - 2;
for (let i = 0; i < argv.length; i += 2) args[argv[i].replace(/^--/, '')] = argv[i + 1];
const g = Number(args.grid), ppc = Number(args.perCell), frames = Number(args.frames);

const eps0 = 8.8541878128e-12, me = 9.109e-31, qe = -1.602e-19, c = 2.998e8;
const dx = 1e-3, L = g * dx;
const yee = args.solver === 'yee';
const dt = yee ? 0.5 * dx / (c * Math.sqrt(3)) : 2e-12;
const wp = 0.05 / dt;                                   // omega_p dt = 0.05
const density = wp * wp * eps0 * me / (qe * qe);
const n = g * g * g * ppc;
const spec = { radius: L, length_y: L, height: L, nr: g, ny: g, nz: g, dt: dt, nparticles: 0, count: n, particle_mass: me,
    particle_charge: qe, geometry: 'cart3d', solver: args.solver, macro_weight: density * L * L * L / n };
const sim = empic.makeCylindricalParticlePusher(spec);

// a regular lattice of particles, displaced along x by a sin(k x): rho = -n0 q a k cos(k x)
const k = 2 * Math.PI / L, amp = 0.02 * dx;
const side = Math.round(Math.cbrt(ppc));
let p = 0;
if (useLoad) {
    // the same plasma made on the GPU: a Kronecker lattice, cold, displaced by amp sin(2 pi x / L)
    p = sim.load({ lattice: true, mode: [1, 0, 0], xamp: [amp, 0, 0] });
} else {
    const position = new Float64Array(3 * n), velocity = new Float64Array(3 * n);
    const per = g * side;
    for (let a = 0; a < per && p < n; a++) for (let b = 0; b < per && p < n; b++) for (let d = 0; d < per && p < n; d++, p++) {
        const x = (a + 0.5) * L / per;
        position[3 * p] = x + amp * Math.sin(k * x);
        position[3 * p + 1] = (b + 0.5) * L / per;
        position[3 * p + 2] = (d + 0.5) * L / per;
    }
    sim.set({ position: position.subarray(0, 3 * p), velocity: velocity.subarray(0, 3 * p) });
}
sim.precalc();

const field = yee ? 'edge_E' : 'E';
function fieldEnergy() {
    const e = sim.readField(field);
    let s = 0;
    for (let i = 0; i < e.length; i += 4) s += e[i] * e[i] + e[i + 1] * e[i + 1] + e[i + 2] * e[i + 2];
    return 0.5 * eps0 * s * dx * dx * dx;
}
// Ex at one node near the crest of the perturbation: its zero crossings give the period.  The electrostatic box records that
// node as a point series on the device (a point on a node gets the node's record exactly) and drains it once per ten frames:
// no grid crosses the host per frame.  Full EM watches the lattice field (edge_E), which the series does not read — the
// series interpolates the node-centred E — so it keeps the read-back per frame.
const node = Math.round(g / 4), probe = 4 * node;
const request = { points: [[node * dx, 0, 0]] };
let last = yee ? sim.readField(field)[probe] : sim.series(request).points[0], crossings = [], t = 0, seen = 0;
function crossing(ex, at) {
    if ((ex > 0) !== (last > 0)) crossings.push(at - 2 * dt * Math.abs(ex) / (Math.abs(ex) + Math.abs(last)));
    last = ex;
}
if (!yee) sim.recordSeries(2, 16, request);              // one row per frame (two sub-steps)
for (let frame = 0; frame < frames; frame++) {
    sim.step();                                             // two sub-steps
    t += 2 * dt;
    if (yee) {
        crossing(sim.readField(field)[probe], t);
    } else if (frame % 10 === 9 || frame === frames - 1) {
        const h = sim.seriesHistory();
        if (h.dropped) throw new Error('the series ring overflowed');
        for (let r = 0; r < h.rows; r++) { seen += 2 * dt; crossing(h.points[8 * r], seen); }
    }
    if (frame % 10 === 0) console.log('frame %d  t = %s ns  field energy %s J', frame, (t * 1e9).toFixed(4), fieldEnergy().toExponential(4));
}
if (!yee) sim.recordSeries(0);
let measured = NaN;
if (crossings.length >= 3) measured = Math.PI * (crossings.length - 1) / (crossings[crossings.length - 1] - crossings[0]);
const expected = wp * Math.cos(k * dx / 2);
// full EM: the exact integer current of the last sub-step (3 int64 per node); its sum over the box is the total
// momentum flux in fixed point, here just shown to be there
let currentNodes = 0;
if (yee) { const J = sim.readField('J_fixed'); for (let i = 0; i < J.length; i++) if (J[i] !== 0n) { currentNodes++; } }
console.log(JSON.stringify({ particles: p, grid: g, solver: args.solver, nonzero_current_entries: currentNodes, omega_measured: measured, omega_scheme: expected, omega_p: wp,
    relative_error: Math.abs(measured - expected) / expected, updates: sim.stats().particle_updates }));
sim.destroy();
