#!/usr/bin/env node
// Y.readMany (crdt_amd/js): the `h[name].get(key)` / `.length` reads of crdt.js:423-430 batched over
// documents. A dozen small cases of tests/golden/{map,array,nested}.json: every batched answer
// deep-equals the facade's own getMap(..).get / .size and getArray(..).get / .length on the same
// document, and Yjs's recorded toJSON().
'use strict';
const fs = require('fs');
const path = require('path');
const assert = require('assert');

const ROOT = path.join(__dirname, '..', '..');
const Y = require(path.join(ROOT, 'crdt_amd', 'js'));
const unhex = (h) => new Uint8Array(Buffer.from(h, 'hex'));
const plain = (v) => (v instanceof Y.AbstractType ? v.toJSON() : v);  // (YMap.get hands out nested types as objects)

assert.strictEqual(typeof Y.readMany, 'function');
const cases = ['map', 'array', 'nested'].flatMap((s) => JSON.parse(fs.readFileSync(path.join(ROOT, 'tests', 'golden', s + '.json'))).cases.slice(0, 4));
assert.strictEqual(cases.length, 12);
const reqs = [], want = [];
for (const c of cases) {
  const d = new Y.Doc({ clientID: 0x7ffffff0 });
  for (const u of c.updates) Y.applyUpdate(d, unhex(u));
  for (const [root, kind] of Object.entries(c.roots)) {
    const j = c.json[root];
    if (kind === 'map') {
      for (const [k, v] of Object.entries(j)) { reqs.push({ doc: d, op: 'mapGet', root, key: k }); want.push(v); }
      reqs.push({ doc: d, op: 'mapGet', root, key: 'no such key' }); want.push(undefined);
      reqs.push({ doc: d, op: 'mapSize', root }); want.push(null);  // (size counts `undefined` entries, toJSON drops them: the facade decides)
      reqs.push({ doc: d, op: 'arrayLength', root, other: true }); want.push(0);  // (the other kind: the facade, as Yjs, refuses to define it)
    } else {
      j.forEach((v, i) => { reqs.push({ doc: d, op: 'arrayGet', root, index: i }); want.push(v === null ? null : v); });
      reqs.push({ doc: d, op: 'arrayGet', root, index: j.length }); want.push(undefined);
      reqs.push({ doc: d, op: 'arrayLength', root }); want.push(j.length);
      reqs.push({ doc: d, op: 'mapSize', root, other: true }); want.push(0);
    }
  }
}
const got = Y.readMany(reqs);
assert.strictEqual(got.length, reqs.length);
got.forEach((v, i) => {
  const q = reqs[i];
  if (q.other) { assert.strictEqual(v, 0, 'request ' + i); return; }
  const single = q.op === 'mapGet' ? plain(q.doc.getMap(q.root).get(q.key)) : q.op === 'mapSize' ? q.doc.getMap(q.root).size
    : q.op === 'arrayGet' ? q.doc.getArray(q.root).get(q.index) : q.doc.getArray(q.root).length;
  assert.deepStrictEqual(v, single, 'request ' + i + ' against the facade');
  if (want[i] !== null && !(q.op === 'arrayGet' && v === undefined)) assert.deepStrictEqual(v, want[i], 'request ' + i + ' against Yjs');
});
// a nested target, a repeated doc, no request, bad arguments
const d = new Y.Doc({ clientID: 7 });
const l = new Y.Array();
d.getMap('users').set('list', l);
l.push(['a', 'b']);
d.getMap('users').set('n', 5);
assert.deepStrictEqual(Y.readMany([
  { doc: d, op: 'arrayGet', root: 'users', parentKey: 'list', index: 1 }, { doc: d, op: 'arrayLength', root: 'users', parentKey: 'list' },
  { doc: d, op: 'mapGet', root: 'users', key: 'list' }, { doc: d, op: 'mapGet', root: 'users', key: 'n' }, { doc: d, op: 'mapSize', root: 'users' },
  { doc: d, op: 'mapSize', root: 'users', parentKey: 'list' }]), ['b', 2, ['a', 'b'], 5, 2, 0]);
assert.deepStrictEqual(Y.readMany([]), []);
assert.throws(() => Y.readMany([{ doc: d, op: 'mapHas', root: 'users', key: 'n' }]), TypeError);
assert.throws(() => Y.readMany([{ doc: d, op: 'mapGet', root: 'users' }]), TypeError);
assert.throws(() => Y.readMany([{ doc: d, op: 'arrayGet', root: 'users' }]), TypeError);
console.log('napi docs read ok:', got.length, 'requests');
