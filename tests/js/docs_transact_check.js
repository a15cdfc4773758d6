#!/usr/bin/env node
// Y.transactMany (crdt_amd/js): Y.writeMany for queues whose ops depend on one another, as
// crdt.js:329-355 (execBatch) runs one per document. The 60 recorded Yjs 13.5.16 op scripts
// (tests/golden/ops.json) run as 60 documents: between the recorded `apply` steps a script's
// consecutive local ops are cut into chunks of at most 8, round k applies every script's k-th event
// through Y.applyUpdatesMulti or issues every chunk through ONE Y.transactMany; after every round each
// document's state is the one recorded behind its chunk's last op. Then: a type set and pushed into in
// one call, the updates a call returns are what takeLocalUpdate collects, a failed op reports its
// message and an observer on a written map fires once per call.
'use strict';
const fs = require('fs');
const path = require('path');
const assert = require('assert');

const ROOT = path.join(__dirname, '..', '..');
const Y = require(path.join(ROOT, 'crdt_amd', 'js'));
const { decodeAny } = require(path.join(ROOT, 'crdt_amd', 'js', 'any.js'));
const unhex = (h) => new Uint8Array(Buffer.from(h, 'hex'));
const hex = (u) => Buffer.from(u).toString('hex');

assert.strictEqual(typeof Y.transactMany, 'function');
const cases = JSON.parse(fs.readFileSync(path.join(ROOT, 'tests', 'golden', 'ops.json'))).cases;
assert.strictEqual(cases.length, 60);
const docs = cases.map((c) => new Y.Doc({ clientID: c.client }));
const opOf = (doc, s) => {
  const parentKey = s.parent_key === null ? undefined : s.parent_key;
  if (s.op === 'map_set') return { doc, op: 'mapSet', root: s.root, parentKey, key: s.key, value: decodeAny(unhex(s.any))[0] };
  if (s.op === 'map_set_type') return { doc, op: 'mapSetType', root: s.root, parentKey, key: s.key, type: s.type === 0 ? 'array' : 'map' };
  if (s.op === 'map_delete') return { doc, op: 'mapDelete', root: s.root, parentKey, key: s.key };
  if (s.op === 'array_insert') return { doc, op: 'arrayInsert', root: s.root, parentKey, index: s.index, content: s.anys.map((a) => decodeAny(unhex(a))[0]) };
  assert.strictEqual(s.op, 'array_delete');
  return { doc, op: 'arrayDelete', root: s.root, parentKey, index: s.index, length: s.length };
};
// per script: its events, an `apply` step or a chunk of at most 8 local steps
const events = cases.map((c) => {
  const ev = [];
  for (const s of c.steps) {
    const last = ev[ev.length - 1];
    if (s.op === 'apply') ev.push(s);
    else if (Array.isArray(last) && last.length < 8) last.push(s);
    else ev.push([s]);
  }
  return ev;
});
let written = 0, chunks = 0;
const rounds = Math.max(...events.map((ev) => ev.length));
for (let k = 0; k < rounds; ++k) {
  const live = events.map((ev, i) => [docs[i], ev[k], cases[i].name]).filter(([, e]) => e !== undefined);
  const applies = live.filter(([, e]) => !Array.isArray(e));
  if (applies.length) Y.applyUpdatesMulti(applies.map(([d]) => d), applies.map(([, s]) => unhex(s.update)));
  const local = live.filter(([, e]) => Array.isArray(e));
  if (local.length) {
    const ops = [];
    for (const [d, chunk] of local) for (const s of chunk) ops.push(opOf(d, s));
    const res = Y.transactMany(ops);
    assert.strictEqual(res.length, ops.length);
    res.forEach((r) => { assert.strictEqual(r.error, null, 'round ' + k); assert.ok(r.update instanceof Uint8Array); });
    written += ops.length;
    chunks += local.length;
  }
  for (const [d, e, name] of live) {
    const s = Array.isArray(e) ? e[e.length - 1] : e;
    assert.strictEqual(hex(Y.encodeStateAsUpdate(d)), s.state, name + ' round ' + k + ' ' + s.op);
  }
}
assert.strictEqual(chunks, 302);
cases.forEach((c, i) => {
  assert.deepStrictEqual(JSON.parse(JSON.stringify(docs[i].getMap('users').toJSON())), c.json.users, c.name);
  assert.deepStrictEqual(JSON.parse(JSON.stringify(docs[i].getArray('messages').toArray())), c.json.messages, c.name);
});

// crdt.js:422-431 in one call — a fresh Y.Array under a key and pushes into it — beside two sets of one
// key; observers: one event per call and written map
const a = new Y.Doc({ clientID: 11 }), b = new Y.Doc({ clientID: 12 });
a.getMap('users').set('seed', 1);
b.getMap('users').set('seed', 1);
Y.trackLocalUpdates(a);
const seen = [];
a.getMap('users').observe((ev, tr) => seen.push(['a', Array.from(ev.keysChanged).sort(), tr.local]));
b.getMap('users').observe((ev) => seen.push(['b', Array.from(ev.keysChanged).sort()]));
const res = Y.transactMany([
  { doc: a, op: 'mapSetType', root: 'users', key: 'list', type: 'array' }, { doc: a, op: 'arrayPush', root: 'users', parentKey: 'list', content: ['m', 2] },
  { doc: b, op: 'mapSet', root: 'users', key: 'seed', value: 2 }, { doc: a, op: 'arrayPush', root: 'users', parentKey: 'list', content: [3] },
  { doc: b, op: 'mapSet', root: 'users', key: 'seed', value: 3 }, { doc: a, op: 'arrayDelete', root: 'users', parentKey: 'list', index: 1, length: 1 },
  { doc: b, op: 'mapDelete', root: 'users', key: 'seed' }, { doc: b, op: 'mapDelete', root: 'users', key: 'seed' },
  { doc: a, op: 'arrayInsert', root: 'users', parentKey: 'list', index: 7, content: ['past the end'] }]);
assert.deepStrictEqual(seen, [['a', ['list'], true], ['b', ['seed']]]);
assert.deepStrictEqual(res.map((r) => r.update.length > 0), [true, true, true, true, true, true, true, false, false]);
assert.deepStrictEqual(res.map((r) => r.error === null), [true, true, true, true, true, true, true, true, false]);
assert.ok(/Length exceeded/.test(res[8].error), res[8].error);
assert.deepStrictEqual(a.getMap('users').toJSON(), { seed: 1, list: ['m', 3] });
assert.deepStrictEqual(b.getMap('users').toJSON(), {});
assert.strictEqual(hex(Y.takeLocalUpdate(a)), hex(Y.mergeUpdates([0, 1, 3, 5].map((i) => res[i].update))));
// the same ops through the facade's own calls give the same document
const t = new Y.Doc({ clientID: 11 });
t.getMap('users').set('seed', 1);
const list = new Y.Array();
t.getMap('users').set('list', list);
list.push(['m', 2]);
list.push([3]);
list.delete(1, 1);
assert.strictEqual(hex(Y.encodeStateAsUpdate(a)), hex(Y.encodeStateAsUpdate(t)));
assert.deepStrictEqual(Y.transactMany([]), []);
assert.throws(() => Y.transactMany([{ doc: a, op: 'mapHas', root: 'users', key: 'n' }]), TypeError);
assert.throws(() => Y.transactMany({}), TypeError);
console.log('napi docs transact ok:', written, 'ops in', chunks, 'chunks');
