#!/usr/bin/env node
// Y.encodeStatesAsUpdates (crdt_amd/js): the sync responder of crdt.js:286-291 batched over peers.
// Three docs of tests/golden/sync.json and five state vectors: every reply equals the per-pair
// Y.encodeStateAsUpdate of the same facade, and Yjs's recorded reply.
'use strict';
const fs = require('fs');
const path = require('path');
const assert = require('assert');

const ROOT = path.join(__dirname, '..', '..');
const Y = require(path.join(ROOT, 'crdt_amd', 'js'));
const hex = (u) => Buffer.from(u).toString('hex');
const unhex = (h) => new Uint8Array(Buffer.from(h, 'hex'));

assert.strictEqual(typeof Y.encodeStatesAsUpdates, 'function');
const cases = JSON.parse(fs.readFileSync(path.join(ROOT, 'tests', 'golden', 'sync.json'))).cases;
const pick = (name) => cases.find((c) => c.name === name);
const used = [pick('wave_steps'), pick('sv_edges'), pick('map_key_reset')];
const docs = used.map((c) => {
  const d = new Y.Doc({ clientID: 0x7ffffff0 });
  for (const u of c.updates) Y.applyUpdate(d, unhex(u));
  return d;
});
// five pairs over three docs (a doc repeats; one peer asks for the full state)
const pairs = [[0, used[0].replies[4]], [1, used[1].replies[2]], [2, used[2].replies[1]], [0, used[0].replies[8]], [1, null]];
const got = Y.encodeStatesAsUpdates(pairs.map(([i]) => docs[i]), pairs.map(([, r]) => (r ? unhex(r.sv) : null)));
assert.strictEqual(got.length, pairs.length);
pairs.forEach(([i, r], k) => {
  assert.ok(got[k] instanceof Uint8Array);
  const single = r ? Y.encodeStateAsUpdate(docs[i], unhex(r.sv)) : Y.encodeStateAsUpdate(docs[i]);
  assert.strictEqual(hex(got[k]), hex(single), 'pair ' + k);
  assert.strictEqual(hex(got[k]), r ? r.update : used[i].state, 'pair ' + k + ' against Yjs');
});
assert.deepStrictEqual(Y.encodeStatesAsUpdates([], []), []);
assert.throws(() => Y.encodeStatesAsUpdates(docs, [null]), TypeError);
console.log('napi sync ok:', pairs.length, 'pairs');
