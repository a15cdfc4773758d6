#!/usr/bin/env node
// Y.writeMany (crdt_amd/js): the `set` / `del` / `push` / `insert` / `cut` of crdt.js:423-611 batched
// over documents. The 60 recorded Yjs 13.5.16 op scripts (tests/golden/ops.json) run in lockstep as 60
// documents: round k applies every script's `apply` step through Y.applyUpdatesMulti and issues every
// other step through one Y.writeMany; after every round each document's state is the recorded one.
// Then: the updates a call returns are what takeLocalUpdate collects, a failed op reports its message
// and an observer on a written map fires once per call.
'use strict';
const fs = require('fs');
const path = require('path');
const assert = require('assert');

const ROOT = path.join(__dirname, '..', '..');
const Y = require(path.join(ROOT, 'crdt_amd', 'js'));
const { decodeAny } = require(path.join(ROOT, 'crdt_amd', 'js', 'any.js'));
const unhex = (h) => new Uint8Array(Buffer.from(h, 'hex'));
const hex = (u) => Buffer.from(u).toString('hex');

assert.strictEqual(typeof Y.writeMany, 'function');
const cases = JSON.parse(fs.readFileSync(path.join(ROOT, 'tests', 'golden', 'ops.json'))).cases;
assert.strictEqual(cases.length, 60);
const docs = cases.map((c) => new Y.Doc({ clientID: c.client }));
const opOf = (doc, s) => {
  const parentKey = s.parent_key === null ? undefined : s.parent_key;
  if (s.op === 'map_set') return { doc, op: 'mapSet', root: s.root, key: s.key, value: decodeAny(unhex(s.any))[0] };
  if (s.op === 'map_set_type') return { doc, op: 'mapSetType', root: s.root, key: s.key, type: s.type === 0 ? 'array' : 'map' };
  if (s.op === 'map_delete') return { doc, op: 'mapDelete', root: s.root, key: s.key };
  if (s.op === 'array_insert') return { doc, op: 'arrayInsert', root: s.root, parentKey, index: s.index, content: s.anys.map((a) => decodeAny(unhex(a))[0]) };
  assert.strictEqual(s.op, 'array_delete');
  return { doc, op: 'arrayDelete', root: s.root, parentKey, index: s.index, length: s.length };
};
let written = 0;
const rounds = Math.max(...cases.map((c) => c.steps.length));
for (let k = 0; k < rounds; ++k) {
  const live = cases.map((c, i) => [docs[i], c.steps[k], c.name]).filter(([, s]) => s !== undefined);
  const applies = live.filter(([, s]) => s.op === 'apply');
  if (applies.length) Y.applyUpdatesMulti(applies.map(([d]) => d), applies.map(([, s]) => unhex(s.update)));
  const local = live.filter(([, s]) => s.op !== 'apply');
  if (local.length) {
    const res = Y.writeMany(local.map(([d, s]) => opOf(d, s)));
    assert.strictEqual(res.length, local.length);
    res.forEach((r, i) => { assert.strictEqual(r.error, null, local[i][2] + ' round ' + k); assert.ok(r.update instanceof Uint8Array); });
    written += local.length;
  }
  for (const [d, s, name] of live) assert.strictEqual(hex(Y.encodeStateAsUpdate(d)), s.state, name + ' round ' + k + ' ' + s.op);
}
cases.forEach((c, i) => {
  assert.deepStrictEqual(JSON.parse(JSON.stringify(docs[i].getMap('users').toJSON())), c.json.users, c.name);
  assert.deepStrictEqual(JSON.parse(JSON.stringify(docs[i].getArray('messages').toArray())), c.json.messages, c.name);
});

// observers: one event per call and written map, however many of its keys the call wrote
const a = new Y.Doc({ clientID: 11 }), b = new Y.Doc({ clientID: 12 });
a.getMap('users').set('seed', 1);
b.getMap('users').set('seed', 1);
Y.trackLocalUpdates(a);
const events = [];
a.getMap('users').observe((ev, tr) => events.push(['a', Array.from(ev.keysChanged).sort(), tr.local]));
b.getMap('users').observe((ev) => events.push(['b', Array.from(ev.keysChanged).sort()]));
const res = Y.writeMany([
  { doc: a, op: 'mapSet', root: 'users', key: 'x', value: { n: 1 } }, { doc: b, op: 'mapDelete', root: 'users', key: 'seed' },
  { doc: a, op: 'mapSet', root: 'users', key: 'y', value: 'two' }, { doc: a, op: 'arrayPush', root: 'messages', content: ['m', 2] },
  { doc: a, op: 'arrayInsert', root: 'messages', index: 7, content: ['past the end'] }, { doc: b, op: 'mapDelete', root: 'users', key: 'absent' }]);
assert.deepStrictEqual(events, [['a', ['x', 'y'], true], ['b', ['seed']]]);
assert.deepStrictEqual(res.map((r) => r.update.length > 0), [true, true, true, true, false, false]);
assert.deepStrictEqual(res.map((r) => r.error === null), [true, true, true, true, false, true]);
assert.ok(/Length exceeded/.test(res[4].error), res[4].error);
assert.deepStrictEqual(a.getMap('users').toJSON(), { seed: 1, x: { n: 1 }, y: 'two' });
assert.deepStrictEqual(a.getArray('messages').toArray(), ['m', 2]);
assert.deepStrictEqual(b.getMap('users').toJSON(), {});
assert.strictEqual(hex(Y.takeLocalUpdate(a)), hex(Y.mergeUpdates([res[0].update, res[2].update, res[3].update])));
assert.strictEqual(events.length, 2);
assert.deepStrictEqual(Y.writeMany([]), []);
assert.throws(() => Y.writeMany([{ doc: a, op: 'mapHas', root: 'users', key: 'n' }]), TypeError);
assert.throws(() => Y.writeMany([{ doc: a, op: 'mapSetType', root: 'users', key: 'n' }]), TypeError);
assert.throws(() => Y.writeMany([{ doc: a, op: 'arrayPush', root: 'messages' }]), TypeError);
console.log('napi docs write ok:', written, 'ops');
