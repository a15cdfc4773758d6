#!/usr/bin/env node
// Y.cachesToJSON (crdt_amd/js): the open / refresh loop of crdt.js:201-216, 297-305 batched over
// documents, the index map read on the device. Every case of tests/golden/cache.json as one fleet:
// the batched objects deep-equal the `c` Yjs 13.5.16 built, and the object the same loop builds
// through the facade's own getMap / getArray / toJSON.
'use strict';
const fs = require('fs');
const path = require('path');
const assert = require('assert');

const ROOT = path.join(__dirname, '..', '..');
const Y = require(path.join(ROOT, 'crdt_amd', 'js'));
const unhex = (h) => new Uint8Array(Buffer.from(h, 'hex'));

assert.strictEqual(typeof Y.cachesToJSON, 'function');
assert.strictEqual(typeof Y.cachesToJSONText, 'function');
const cases = JSON.parse(fs.readFileSync(path.join(ROOT, 'tests', 'golden', 'cache.json'))).cases;
const fresh = (c) => {
  const d = new Y.Doc({ clientID: 0x7ffffff0 });
  for (const u of c.updates) Y.applyUpdate(d, unhex(u));
  return d;
};
function loop(doc, index) { // crdt.js's loop, through the facade
  const ix = doc.getMap(index).toJSON();
  const c = {};
  for (const [key, val] of Object.entries(ix)) {
    const h = val == 'map' ? doc.getMap(key) : doc.getArray(key); // eslint-disable-line eqeqeq
    c[key] = h.toJSON();
  }
  return c;
}
const byIndex = new Map();
for (const c of cases) byIndex.set(c.index, (byIndex.get(c.index) || []).concat([c]));
let members = 0;
for (const [index, cs] of byIndex) {
  const docs = cs.map(fresh);
  const got = index === 'ix' ? Y.cachesToJSON(docs) : Y.cachesToJSON(docs, index);
  const texts = Y.cachesToJSONText(docs, index);
  assert.strictEqual(got.length, docs.length);
  got.forEach((v, i) => {
    // an index entry whose value is undefined: Yjs's toJSON lists it, the facade's object (through JSON) cannot
    const undef = cs[i].entries.filter((e) => e.content === '017f').map((e) => e.name);
    const want = cs[i].c;
    assert.deepStrictEqual(v, want, cs[i].name + ' against Yjs');
    const mine = loop(fresh(cs[i]), index);
    for (const n of undef) mine[n] = v[n];
    assert.deepStrictEqual(v, mine, cs[i].name + ' against the loop through the facade');
    assert.deepStrictEqual(JSON.parse(texts[i]), v);
    members += Object.keys(v).length;
  });
}
// a repeated doc, no doc, bad arguments
const d = fresh(cases.find((c) => c.name === 'basic'));
const basic = cases.find((c) => c.name === 'basic').c;
assert.deepStrictEqual(Y.cachesToJSON([d, d]), [basic, basic]);
assert.deepStrictEqual(Y.cachesToJSON([d], 'absent'), [{}]);
assert.deepStrictEqual(Y.cachesToJSON([]), []);
assert.throws(() => Y.cachesToJSON(d), TypeError);
assert.throws(() => Y.cachesToJSON([d], 5), TypeError);
console.log('napi docs cache ok:', cases.length, 'documents,', members, 'members');
