#!/usr/bin/env node
// Golden vectors for the doc-less update store (TEST INFRASTRUCTURE ONLY; runs in the build
// container with the in-image Yjs 13.5.16, see load_yjs.js): Y.encodeStateVectorFromUpdate and
// Y.mergeUpdates for inputs the older corpora lack —
//   diff:     diffUpdate outputs whose first clock is not 0;
//   gaps:     mergeUpdates of non-adjacent updates (Skips in the middle, and a client that no longer
//             starts at clock 0), and those outputs as inputs again;
//   gc:       GC structs (the children of a deleted shared type);
//   ds_only:  updates that hold a delete set and no struct;
//   overlap:  two updates of one client with overlapping clocks;
//   hand:     bytes Yjs reads but never writes: an update that opens with a Skip at clock 0, a Skip
//             first in a later client, an empty section, the empty update;
//   sections: the two-sections-of-one-client / ascending-order updates of edges.json.
// Every case records its input updates, Yjs's state vector of each, and Yjs's mergeUpdates of the
// list (raw, and with the delete set in the canonical descending client order).
// Usage: node gen_update_store_fixtures.js <golden_dir>   → <golden_dir>/update_store.json
'use strict';
const fs = require('fs');
const path = require('path');
const { loadYjs } = require('./load_yjs.js');
const { canonicalUpdate, hex } = require('./v1.js');

const Y = loadYjs();
const unhex = (h) => new Uint8Array(Buffer.from(h, 'hex'));
const cases = [];

function add(name, kind, ups) {
  const merged = Y.mergeUpdates(ups);
  cases.push({ name, kind, updates: ups.map(hex), svs: ups.map((u) => hex(Y.encodeStateVectorFromUpdate(u))),
               merged: hex(canonicalUpdate(merged)), merged_raw: hex(merged), merged_sv: hex(Y.encodeStateVectorFromUpdate(merged)) });
}

// a replica whose every transaction is kept as its own update
function replica(clientID, gc) {
  const d = new Y.Doc({ gc: gc !== false });
  d.clientID = clientID;
  const log = [];
  d.on('update', (u) => log.push(u));
  return { d, log };
}

// ---- three replicas, one transaction per update, a few exchanges
const A = replica(11); const B = replica(700); const C = replica(40000);
{
  const arr = (r) => r.d.getArray('messages'); const map = (r) => r.d.getMap('users');
  arr(A).push(['a0', 'a1']); map(A).set('k', 1); arr(A).insert(1, [7, 8, 9]);
  arr(B).push(['b0']); map(B).set('k', 'bee');
  Y.applyUpdate(B.d, Y.encodeStateAsUpdate(A.d));
  arr(B).delete(0, 2); arr(B).push([{ x: 1 }]);
  arr(C).unshift(['c0', 'c1', 'c2']); Y.applyUpdate(C.d, Y.encodeStateAsUpdate(B.d));
  map(C).delete('k'); arr(C).insert(2, ['mid']); arr(A).push(['a-late']); map(A).set('z', null);
}
// the logs: A's five transactions; B's and C's also hold the remote states they applied
const la = A.log; const lb = B.log; const lc = C.log;

// ---- diff: what a peer that holds part of a document is sent
{
  const full = Y.encodeStateAsUpdate(C.d);
  const svA = Y.encodeStateVector(A.d);
  const svHalf = Y.encodeStateVectorFromUpdate(Y.mergeUpdates(la.slice(0, 2)));
  add('diff_vs_A', 'diff', [Y.diffUpdate(full, svA)]);
  add('diff_vs_half', 'diff', [Y.diffUpdate(full, svHalf), Y.diffUpdate(Y.encodeStateAsUpdate(A.d), svHalf)]);
  add('diff_pair_then_full', 'diff', [Y.diffUpdate(full, svA), Y.encodeStateAsUpdate(A.d)]);
}
// ---- gaps: a log with holes
{
  add('gap_middle', 'gaps', [la[0], la[2]]);
  add('gap_middle_rev', 'gaps', [la[2], la[0]]);
  add('gap_start', 'gaps', [la[1], la[3], lb[0]]);
  add('gap_two_clients', 'gaps', [la[0], la[2], lb[0], lb[lb.length - 1], lc[lc.length - 1]]);
  const holed = Y.mergeUpdates([la[0], la[2]]);       // holds a Skip
  const late = Y.mergeUpdates([la[1], la[3]]);        // starts past clock 0, holds a Skip
  add('gap_refilled', 'gaps', [holed, la[1]]);
  add('gap_inputs_with_skips', 'gaps', [holed, late, lb[0]]);
  add('gap_whole_log', 'gaps', la.concat(lb, lc));
}
// ---- gc: the children of a deleted shared type become GC structs
{
  const G = replica(5000, true);
  const m = G.d.getMap('users');
  const inner = new Y.Array();
  m.set('list', inner);
  inner.push([1, 2, 3]); inner.push(['x']);
  m.delete('list');
  G.d.getArray('messages').push(['after']);
  const state = Y.encodeStateAsUpdate(G.d);
  add('gc_state', 'gc', [state]);
  add('gc_with_log', 'gc', [state, G.log[0], G.log[G.log.length - 1]]);
  add('gc_diff', 'gc', [Y.diffUpdate(state, Y.encodeStateVectorFromUpdate(G.log[0])), G.log[0]]);
}
// ---- ds_only: a delete is an update without structs
{
  const dels = A.log.concat(B.log, C.log).filter((u) => u[0] === 0 && u.length > 2);
  if (dels.length < 2) throw new Error('expected delete-only updates in the logs');
  add('ds_only_one', 'ds_only', [dels[0]]);
  add('ds_only_all', 'ds_only', dels);
  add('ds_only_with_structs', 'ds_only', [dels[0], la[0], dels[dels.length - 1]]);
}
// ---- overlap: the same client's clocks twice
{
  const O = replica(77);
  const arr = O.d.getArray('messages');
  arr.push(['p', 'q', 'r']);
  const early = Y.encodeStateAsUpdate(O.d);
  arr.push(['s']); arr.insert(1, ['t', 'u']);
  const late = Y.encodeStateAsUpdate(O.d);
  const tail = Y.diffUpdate(late, Y.encodeStateVectorFromUpdate(Y.mergeUpdates([O.log[0]])));
  const cut = Y.diffUpdate(late, new Uint8Array([1, 77, 2]));  // from inside the first struct
  add('overlap_early_late', 'overlap', [early, late]);
  add('overlap_late_early', 'overlap', [late, early]);
  add('overlap_cut', 'overlap', [early, cut, tail]);
}
// ---- hand: bytes Yjs reads but never writes
{
  const h = (s) => unhex(s.replace(/\s+/g, ''));
  const item = '08 01 01 61 01 7d 01';  // ContentAny [1] in root "a", no origins
  add('hand_empty_update', 'hand', [h('00 00')]);
  add('hand_open_skip_clock0', 'hand', [h('01 01 05 00 0a 03 00')]);
  add('hand_open_skip_then_item', 'hand', [h('01 02 05 00 0a 03' + item + '00')]);
  add('hand_open_skip_clock4', 'hand', [h('01 02 05 04 0a 03' + item + '00')]);
  add('hand_skip_first_in_second_client', 'hand', [h('02 01 09 00' + item + '02 05 00 0a 02' + item + '00')]);
  add('hand_item_skip_item', 'hand', [h('01 03 05 00' + item + '0a 02' + item + '00')]);
  add('hand_empty_section', 'hand', [h('02 00 09 00 01 05 00' + item + '00')]);
  add('hand_same_client_twice', 'hand', [h('02 01 05 00' + item + '01 05 07' + item + '00')]);
  add('hand_same_client_twice_late_first', 'hand', [h('02 01 05 03' + item + '01 05 00' + item + '00')]);
}
// ---- sections: edges.json's non-canonical updates
{
  const dir = process.argv[2] || path.join(__dirname, '..');
  const edges = JSON.parse(fs.readFileSync(path.join(dir, 'edges.json'))).cases.filter((c) => c.kind === 'sections' && /_[01]$/.test(c.name));  // (two of each shape)
  for (const c of edges) add('sections_' + c.name, 'sections', [unhex(c.update)].concat(c.others.map(unhex)));
}

const dir = process.argv[2] || path.join(__dirname, '..');
const f = path.join(dir, 'update_store.json');
fs.writeFileSync(f, JSON.stringify({ generator: 'tests/golden/gen/gen_update_store_fixtures.js', yjs: '13.5.16', cases }));
console.log(f, cases.length, 'cases', fs.statSync(f).size, 'bytes');
