#!/usr/bin/env node
// Sync-reply fixture generator (TEST INFRASTRUCTURE ONLY; runs in the build container, never on the
// GPU box). The responder of crdt.js:286-291 answers a peer's state vector with
// Y.encodeStateAsUpdate(doc, sv): per client block a new header, the struct holding the peer's
// clock written at an offset (Item.write(encoder, offset), Y@80416) and the structs behind it.
// Every case here is one small document built by the real Yjs 13.5.16 and a list of state vectors
// with the reply Yjs gives (delete set in 13.6 canonical order, v1.js canonicalUpdate), chosen so
// that the cut falls into every kind of struct ycrdt_docs_diff re-encodes.
//
// Usage: node gen_sync_fixtures.js <out_dir>   → <out_dir>/sync.json
'use strict';
const fs = require('fs');
const path = require('path');
const { loadYjs } = require('./load_yjs.js');
const { canonicalUpdate, hex } = require('./v1.js');

const Y = loadYjs();

function newDoc(client) { const d = new Y.Doc(); d.clientID = client; return d; }
function vu(out, v) { while (v > 127) { out.push(128 | (v % 128)); v = Math.floor(v / 128); } out.push(v); }
// a state vector from [[client, clock], ...], in the order given
function sv(entries) {
  const out = [];
  vu(out, entries.length);
  for (const [c, k] of entries) { vu(out, c); vu(out, k); }
  return Uint8Array.from(out);
}

const cases = [];
// updates: what a replica receives (every source doc's full state); svs: state vectors to answer
function add(name, sources, svs, note) {
  const updates = sources.map((d) => Y.encodeStateAsUpdate(d));
  const m = newDoc(0x7ffffff0);
  for (const u of updates) Y.applyUpdate(m, u);
  const c = {
    name, note, updates: updates.map(hex),
    state: hex(canonicalUpdate(Y.encodeStateAsUpdate(m))),
    replies: svs.map((s) => {
      // (lib0 0.2.42 writes strings with encodeURIComponent: a lone surrogate makes Yjs itself throw)
      try { return { sv: hex(s), update: hex(canonicalUpdate(Y.encodeStateAsUpdate(m, s))) }; }
      catch (e) { return { sv: hex(s), update: null, throws: String(e.name) }; }
    }),
  };
  cases.push(c);
}
// the two replicas exchange everything
function syncDocs(a, b) {
  Y.applyUpdate(b, Y.encodeStateAsUpdate(a, Y.encodeStateVector(b)));
  Y.applyUpdate(a, Y.encodeStateAsUpdate(b, Y.encodeStateVector(a)));
}

{ // one String item "abcd" cut at 1, 2 and 3
  const d = newDoc(1);
  d.getText('t').insert(0, 'abcd');
  add('text_abcd', [d], [sv([[1, 1]]), sv([[1, 2]]), sv([[1, 3]]), sv([[1, 0]]), sv([[1, 4]])], 'ContentString cut at 1, 2, 3');
}
{ // UTF-16 lengths: é (2 bytes, 1 unit), 漢 (3 bytes, 1 unit), an emoji (4 bytes, a surrogate pair)
  const d = newDoc(2);
  d.getText('t').insert(0, 'aé漢😀b');  // units: a0 é1 漢2 😀3,4 b5
  add('text_unicode', [d], [sv([[2, 1]]), sv([[2, 2]]), sv([[2, 3]]), sv([[2, 5]])], 'cuts before and after the surrogate pair');
  add('text_pair_inside', [d], [sv([[2, 4]])], 'a cut inside the surrogate pair: Yjs 13.5.16 throws URIError; the engine refuses it too');
}
{ // one push([1,2,3]) cut at 1 and 2
  const d = newDoc(3);
  d.getArray('a').push([1, 2, 3]);
  add('push123', [d], [sv([[3, 1]]), sv([[3, 2]])], 'ContentAny cut at 1 and 2');
}
{ // a map key set four times by one client: the merged ContentDeleted run under a parentSub is cut
  const d = newDoc(4);
  const m = d.getMap('m');
  for (let i = 0; i < 4; ++i) m.set('k', i);
  add('map_key_reset', [d], [sv([[4, 1]]), sv([[4, 2]]), sv([[4, 3]])], 'info bit 0x20 kept on a cut item that has an origin');
}
{ // a deleted array run cut in the middle
  const d = newDoc(5);
  const a = d.getArray('a');
  a.push([10, 11, 12, 13, 14, 15]);
  a.delete(1, 4);
  add('deleted_run', [d], [sv([[5, 2]]), sv([[5, 3]]), sv([[5, 4]]), sv([[5, 5]])], 'ContentDeleted run cut in the middle');
}
{ // a nested Y.Array under a map key that is then deleted: GC structs, a cut inside the GC
  const d = newDoc(6);
  const m = d.getMap('m');
  const inner = new Y.Array();
  m.set('list', inner);
  inner.push([1, 2, 3, 4]);
  inner.push(['x']);
  m.delete('list');
  m.set('other', 'v');
  add('nested_gc', [d], [sv([[6, 2]]), sv([[6, 3]]), sv([[6, 4]]), sv([[6, 5]]), sv([[6, 6]])], 'GC struct cut');
}
{ // an item with both origin and right origin, cut
  const d = newDoc(7);
  const a = d.getArray('a');
  a.push(['l']);
  a.push(['r']);
  a.insert(1, ['m0', 'm1', 'm2', 'm3']);
  add('origin_and_right', [d], [sv([[7, 3]]), sv([[7, 4]]), sv([[7, 5]]), sv([[7, 2]])], 'origin and right origin on the cut item');
}
{ // a root-parent first item, cut (ContentJSON is not produced by 13.5.16; strings as any values)
  const d = newDoc(8);
  d.getArray('root-array-name').insert(0, ['x', 'yy', { k: [1, 2] }, 'zzz']);
  add('root_first', [d], [sv([[8, 1]]), sv([[8, 2]]), sv([[8, 3]])], 'the parent (root name) is dropped on the cut item');
}
{ // client ids >= 2^28: the header varuints take 5 bytes
  const a = newDoc(0x10000005), b = newDoc(0xf0000001);
  a.getArray('a').push([1, 2, 3]);
  syncDocs(a, b);
  b.getArray('a').push([4, 5, 6]);
  b.getMap('m').set('k', 'v');
  syncDocs(a, b);
  a.getArray('a').delete(1, 3);
  add('big_clients', [a, b], [sv([[0x10000005, 2]]), sv([[0xf0000001, 1], [0x10000005, 3]]), sv([[0xf0000001, 2]]), sv([[0xf0000001, 4], [0x10000005, 1]])],
      '5-byte client ids');
}
{ // 65 and 130 single-value structs (unshift: no merge): the peer's clock around 64 and 128 structs
  const a = newDoc(9), b = newDoc(10);
  for (let i = 0; i < 65; ++i) a.getArray('a').unshift([i]);
  for (let i = 0; i < 130; ++i) b.getArray('b').unshift([i]);
  const svs = [];
  for (const k of [63, 64, 65]) svs.push(sv([[9, k]]));
  for (const k of [63, 64, 65, 128, 129]) svs.push(sv([[10, k], [9, 65]]));
  svs.push(sv([[9, 64], [10, 129]]));
  add('wave_steps', [a, b], svs, '65 and 130 structs of length 1');
}
{ // state vectors naming unknown clients, clocks past the end, svc == end, and 00
  const a = newDoc(11), b = newDoc(12);
  a.getMap('m').set('x', 1);
  a.getArray('a').push(['p', 'q']);
  syncDocs(a, b);
  b.getArray('a').push(['r', 's']);
  b.getMap('m').delete('x');
  add('sv_edges', [a, b], [
    sv([]), sv([[99, 5]]), sv([[99, 5], [11, 1]]), sv([[11, 3], [12, 3]]), sv([[11, 100], [12, 100]]),
    sv([[11, 3]]), sv([[12, 3]]), sv([[12, 2], [11, 2], [7, 0]]), sv([[11, 0], [12, 0]]),
  ], 'unknown clients, clocks past the end, svc == end, the empty vector');
}

const outDir = process.argv[2] || path.join(__dirname, '..');
fs.writeFileSync(path.join(outDir, 'sync.json'), JSON.stringify({
  generator: 'tests/golden/gen/gen_sync_fixtures.js', yjs: '13.5.16', lib0: '0.2.42', cases,
}, null, 1) + '\n');
console.log('sync.json:', cases.length, 'cases,', cases.reduce((n, c) => n + c.replies.length, 0), 'replies');
