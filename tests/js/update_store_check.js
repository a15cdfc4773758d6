#!/usr/bin/env node
// The doc-less update store of the Node facade (crdt_amd/js): Y.encodeStateVectorFromUpdate (the Yjs
// name), Y.encodeStateVectorsFromUpdates and Y.mergeUpdatesGroups against the bytes Yjs 13.5.16
// recorded in tests/golden/merge.json (state vectors of first / last updates, merges of reversed
// inputs and of pairs) and tests/golden/update_store.json.
'use strict';
const fs = require('fs');
const path = require('path');
const assert = require('assert');

const ROOT = path.join(__dirname, '..', '..');
const Y = require(path.join(ROOT, 'crdt_amd', 'js'));
const { canonicalUpdate } = require(path.join(ROOT, 'tests', 'golden', 'gen', 'v1.js'));
const unhex = (h) => new Uint8Array(Buffer.from(h, 'hex'));
const hex = (u) => Buffer.from(u).toString('hex');
const load = (f) => JSON.parse(fs.readFileSync(path.join(ROOT, 'tests', 'golden', f + '.json'))).cases;

for (const f of ['encodeStateVectorFromUpdate', 'encodeStateVectorsFromUpdates', 'mergeUpdatesGroups']) assert.strictEqual(typeof Y[f], 'function', f);

const corpus = new Map();
for (const s of ['kat', 'map', 'array', 'nested']) for (const c of load(s)) corpus.set(s + '/' + c.name, c);

// ---- state vectors: (update, Yjs's bytes)
const ups = [], svs = [];
for (const m of load('merge')) {
  const c = corpus.get(m.set + '/' + m.name);
  const rec = m.diffs.filter((d) => d.src === 'merged').map((d) => d.sv);
  ups.push(unhex(c.updates[0])); svs.push(rec[1]);
  if (c.updates.length >= 2) { ups.push(unhex(c.updates[c.updates.length - 1])); svs.push(rec[2]); }
}
assert.strictEqual(ups.length, 141);
const store = load('update_store');
for (const c of store) {
  c.updates.forEach((u, i) => { ups.push(unhex(u)); svs.push(c.svs[i]); });
  ups.push(unhex(c.merged_raw)); svs.push(c.merged_sv);
}
const got = Y.encodeStateVectorsFromUpdates(ups);
assert.strictEqual(got.length, ups.length);
got.forEach((g, i) => assert.strictEqual(hex(g), svs[i], 'state vector ' + i));
for (const i of [0, 7, 140, 141, ups.length - 1]) assert.strictEqual(hex(Y.encodeStateVectorFromUpdate(ups[i])), svs[i], 'single state vector ' + i);
assert.strictEqual(hex(Y.encodeStateVectorFromUpdate(new Uint8Array([0, 0]))), '00');
assert.deepStrictEqual(Y.encodeStateVectorsFromUpdates([]), []);
assert.throws(() => Y.encodeStateVectorsFromUpdates([ups[0], new Uint8Array([5, 255]), ups[1]]), /Integer out of range/);
assert.throws(() => Y.encodeStateVectorFromUpdate('nope'), TypeError);

// ---- mergeUpdates per group
const groups = [], want = [];
for (const m of load('merge')) {
  const c = corpus.get(m.set + '/' + m.name);
  const u = c.updates.map(unhex);
  groups.push(u); want.push(u.length > 1 ? c.merged : c.merged_raw);
  groups.push(u.slice().reverse()); want.push(u.length > 1 ? hex(canonicalUpdate(unhex(m.rev))) : c.merged_raw);
  if (m.pair) { groups.push(u.slice(0, 2)); want.push(hex(canonicalUpdate(unhex(m.pair)))); }
}
for (const c of store) {
  if (c.kind === 'hand') continue;  // (byte layouts Yjs re-encodes: the state-vector cases above)
  groups.push(c.updates.map(unhex)); want.push(c.updates.length > 1 ? c.merged : c.updates[0]);
}
groups.push([]); want.push('0000');
const merged = Y.mergeUpdatesGroups(groups);
assert.strictEqual(merged.length, groups.length);
merged.forEach((g, i) => assert.strictEqual(hex(g), want[i], 'group ' + i));
for (const i of [0, 1, 5, groups.length - 2]) if (groups[i].length > 1) assert.strictEqual(hex(Y.mergeUpdates(groups[i])), want[i], 'single merge ' + i);
assert.deepStrictEqual(Y.mergeUpdatesGroups([]), []);
assert.throws(() => Y.mergeUpdatesGroups([[ups[0]], 'nope']), TypeError);
assert.throws(() => Y.mergeUpdatesGroups([[ups[0], new Uint8Array([5, 255])]]), /Integer out of range/);
console.log('napi update store ok:', got.length, 'state vectors,', merged.length, 'groups');
