#!/usr/bin/env node
// Y.rootsToJSON (crdt_amd/js): the `c[key] = h[key].toJSON()` refresh of crdt.js:297-305 batched
// over documents. Every case of tests/golden/{map,nested}.json: the batched values deep-equal the
// per-type doc.getMap(name).toJSON() / getArray(name).toJSON() of the same facade and Yjs's
// recorded toJSON().
'use strict';
const fs = require('fs');
const path = require('path');
const assert = require('assert');

const ROOT = path.join(__dirname, '..', '..');
const Y = require(path.join(ROOT, 'crdt_amd', 'js'));
const unhex = (h) => new Uint8Array(Buffer.from(h, 'hex'));

assert.strictEqual(typeof Y.rootsToJSON, 'function');
const cases = ['map', 'nested'].flatMap((s) => JSON.parse(fs.readFileSync(path.join(ROOT, 'tests', 'golden', s + '.json'))).cases);
const docs = [], names = [], kinds = [], want = [];
for (const c of cases) {
  const d = new Y.Doc({ clientID: 0x7ffffff0 });
  for (const u of c.updates) Y.applyUpdate(d, unhex(u));
  for (const [name, kind] of Object.entries(c.roots)) {
    docs.push(d);
    names.push(name);
    kinds.push(kind);
    want.push(c.json[name]);
  }
}
const got = Y.rootsToJSON(docs, names, kinds);
assert.strictEqual(got.length, docs.length);
got.forEach((v, i) => {
  const single = kinds[i] === 'map' ? docs[i].getMap(names[i]).toJSON() : docs[i].getArray(names[i]).toJSON();
  assert.deepStrictEqual(v, single, 'request ' + i + ' against the per-type toJSON');
  assert.deepStrictEqual(v, want[i], 'request ' + i + ' against Yjs');
});
// one kind for all, a repeated doc, no request, bad arguments
const maps = kinds.map((k, i) => (k === 'map' ? i : -1)).filter((i) => i >= 0).slice(0, 5);
assert.deepStrictEqual(Y.rootsToJSON(maps.map((i) => docs[i]), maps.map((i) => names[i]), 'map'), maps.map((i) => want[i]));
assert.deepStrictEqual(Y.rootsToJSON([docs[0], docs[0]], [names[0], 'absent'], [kinds[0], 'array']), [want[0], []]);
assert.deepStrictEqual(Y.rootsToJSON([], [], []), []);
assert.throws(() => Y.rootsToJSON(docs, ['x'], ['map']), TypeError);
assert.throws(() => Y.rootsToJSON([docs[0]], ['x'], ['text']), TypeError);
console.log('napi docs json ok:', got.length, 'requests');
