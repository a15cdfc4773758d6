#!/usr/bin/env node
// Text content through the Node facade (crdt_amd/js): the 16 hand-built ContentString cases of
// tests/golden/text.json (map_empty left out: tests/test_gpu_text.py says why) through Y.applyUpdate,
// Y.encodeStateAsUpdate and Y.mergeUpdates, against what Yjs 13.5.16 recorded. A string cut between
// the two units of a surrogate pair holds U+FFFD on both sides; a state vector whose clock falls
// inside a pair that is not split makes Yjs throw, and the facade too.
'use strict';
const fs = require('fs');
const path = require('path');
const zlib = require('zlib');
const assert = require('assert');

const ROOT = path.join(__dirname, '..', '..');
const Y = require(path.join(ROOT, 'crdt_amd', 'js'));
const { canonicalUpdate, canonicalSv, hex } = require(path.join(ROOT, 'tests', 'golden', 'gen', 'v1.js'));

const raw = JSON.parse(fs.readFileSync(path.join(ROOT, 'tests', 'golden', 'text.json')));
const cat = zlib.inflateSync(Buffer.from(raw.blobs_z, 'base64'));
const blobs = [];
let at = 0;
for (const n of raw.blob_lens) { blobs.push(new Uint8Array(cat.subarray(at, at + n))); at += n; }
assert.strictEqual(at, cat.length);
const val = (x) => (typeof x === 'number' ? blobs[x] : null);  // null: Yjs threw

assert.strictEqual(raw.hand.length, 16);
let splits = 0, thrown = 0, replies = 0;
for (const c of raw.hand) {
  if (c.name === 'map_empty') continue;
  const ups = c.updates.map((i) => blobs[i]);
  const doc = new Y.Doc({ clientID: 0x7ffffff0 });
  for (const u of ups) Y.applyUpdate(doc, u);
  assert.strictEqual(hex(Y.encodeStateAsUpdate(doc)), hex(val(c.state)), c.name + ' state');
  assert.strictEqual(hex(canonicalSv(Y.encodeStateVector(doc))), hex(val(c.sv)), c.name + ' state vector');
  for (const r of c.replies) {
    const want = val(r.update);
    if (want === null) {
      assert.throws(() => Y.encodeStateAsUpdate(doc, blobs[r.sv]), /Yjs throws at this offset/, c.name + ' reply');
      ++thrown;
    } else {
      assert.strictEqual(hex(Y.encodeStateAsUpdate(doc, blobs[r.sv])), hex(want), c.name + ' reply ' + hex(blobs[r.sv]));
      ++replies;
    }
  }
  assert.strictEqual(hex(canonicalUpdate(Y.mergeUpdates(ups))), hex(val(c.merged)), c.name + ' merged');
  assert.strictEqual(hex(canonicalUpdate(Y.mergeUpdates(ups.slice().reverse()))), hex(val(c.merged_rev)), c.name + ' merged reversed');
  if (c.name !== 'map_pair_last') assert.deepStrictEqual(doc.getMap('m').toJSON(), JSON.parse(Buffer.from(blobs[c.json_m]).toString()), c.name + ' m');
  if (c.pair_split) ++splits;
}
assert.ok(splits === 6 && thrown === 7 && replies >= 30, `${splits} ${thrown} ${replies}`);  // (what the fixture holds)
console.log('napi text ok:', splits, 'cases with a split pair,', replies, 'replies,', thrown, 'thrown');
