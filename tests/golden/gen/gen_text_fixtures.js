#!/usr/bin/env node
// Text fixture generator (TEST INFRASTRUCTURE ONLY; runs in the build container, never on the GPU
// box). ContentString is the one content whose length, in UTF-16 code units, is neither its byte
// count nor its character count; a peer that keeps a Y.Text sends strings that are cut at origins,
// by delete-set ranges, by partly known duplicates and by lazy merges, and a cut between the two
// units of a surrogate pair makes Yjs 13.5.16 write U+FFFD on both sides (ContentString.splice).
//
// Seeded concurrent text histories (2-5 replicas, 4 rounds of 5 local ops each and a partial gossip
// of state-vector deltas) and hand-built updates, every one applied, merged and diffed by the real
// Yjs. Half of the seeds never place an index inside a pair ("safe"), the others place indices
// freely ("free"); a quarter add format and embed items, a quarter keep the text under m.doc.
// The merging document never instantiates the text type before its bytes are taken, so Yjs's
// formatting cleanup is no part of the answer.
//
// Every byte string (inputs, Yjs's answers, the JSON texts) is an index into one table, written
// deflated (zlib, level 9) and base64: `blobs_z` is the byte strings back to back, cut by `blob_lens`.
//
// Usage: node gen_text_fixtures.js <out_dir>   → <out_dir>/text.json
'use strict';
const fs = require('fs');
const path = require('path');
const zlib = require('zlib');
const { loadYjs } = require('./load_yjs.js');
const { canonicalUpdate, canonicalSv } = require('./v1.js');

const Y = loadYjs();
const ME = 0x7ffffff0;
const NSEEDS = 48;
const ALPHABET = ['a', 'b', 'é', 'ß', '漢', '€', '😀', '𝄞'];

function mulberry32(a) {
  return () => {
    a = (a + 0x6d2b79f5) | 0;
    let t = Math.imul(a ^ (a >>> 15), 1 | a);
    t = (t + Math.imul(t ^ (t >>> 7), 61 | t)) ^ t;
    return ((t ^ (t >>> 14)) >>> 0) / 4294967296;
  };
}
function newDoc(client) { const d = new Y.Doc(); d.clientID = client; return d; }

// ---- the blob table
const blobs = [];
const blobIndex = new Map();
function blob(u) {
  const b = Buffer.from(u);
  const k = b.toString('latin1');
  if (!blobIndex.has(k)) { blobIndex.set(k, blobs.length); blobs.push(b); }
  return blobIndex.get(k);
}
const text = (s) => blob(Buffer.from(s, 'utf8'));

// ---- what Yjs answers for a list of updates
function bytesOrThrows(f) {
  try { return blob(f()); } catch (e) { return { throws: String(e.name) }; }
}
const hasPair = (s) => /[\ud800-\udbff]/.test(s);
function record(name, kind, updates, svs, extra) {
  const c = Object.assign({ name, kind }, extra, { updates: updates.map(blob) });
  c.update_svs = updates.map((u) => blob(canonicalSv(Y.encodeStateVectorFromUpdate(u))));
  let m;
  try {
    m = newDoc(ME);
    c.parks = false;  // some update waits for a missing dependency on the way
    for (const u of updates) {
      Y.applyUpdate(m, u);
      if (m.store.pendingStructs !== null || m.store.pendingDs !== null) c.parks = true;
    }
    const raw = Y.encodeStateAsUpdate(m);
    c.state_raw = blob(raw);
    c.state = blob(canonicalUpdate(raw));
    c.sv = blob(canonicalSv(Y.encodeStateVector(m)));
    c.pending = m.store.pendingStructs !== null || m.store.pendingDs !== null;
  } catch (e) {
    c.apply_throws = String(e.name);
    return c;
  }
  const r = newDoc(ME);
  for (const u of updates.slice().reverse()) Y.applyUpdate(r, u);
  c.state_rev = blob(canonicalUpdate(Y.encodeStateAsUpdate(r)));
  c.merged = bytesOrThrows(() => canonicalUpdate(Y.mergeUpdates(updates)));
  c.merged_rev = bytesOrThrows(() => canonicalUpdate(Y.mergeUpdates(updates.slice().reverse())));
  const merged = Y.mergeUpdates(updates);
  c.replies = svs.map((s) => ({
    sv: blob(s),
    update: bytesOrThrows(() => canonicalUpdate(Y.encodeStateAsUpdate(m, s))),
    diff: bytesOrThrows(() => canonicalUpdate(Y.diffUpdate(merged, s))),
  }));
  // reads last: only now may the merging document instantiate a type (as a list, never as a text)
  const jm = JSON.stringify(m.getMap('m').toJSON());
  const arr = m.getArray('t');
  const jt = JSON.stringify(arr.toJSON());
  c.json_m = text(jm);
  c.json_t = text(jt);
  c.len_t = arr.length;
  c.has_fffd = jm.includes('�') || jt.includes('�');
  return c;
}

// ---- seeded histories
function randomHistory(seed) {
  const g = mulberry32(0x7e87 + seed * 7919);
  const ri = (n) => Math.floor(g() * n);
  const free = seed % 2 === 1;
  const fmt = (seed >> 1) % 4 === 0;     // format and embed items
  const nested = (seed >> 1) % 4 === 1;  // the text under key `doc` of root map `m`
  const nrep = 2 + ri(4);
  const docs = [];
  for (let i = 0; i < nrep; ++i) docs.push(newDoc(1 + seed * 8 + i));
  const updates = [];
  if (nested) {
    docs[0].getMap('m').set('doc', new Y.Text());
    const u = Y.encodeStateAsUpdate(docs[0]);
    updates.push(u);
    for (let i = 1; i < nrep; ++i) Y.applyUpdate(docs[i], u);
  }
  const textOf = (d) => (nested ? d.getMap('m').get('doc') : d.getText('t'));
  // the UTF-16 units of a text as Yjs counts them (an embed is one unit)
  const unitsOf = (t) => {
    let s = '';
    for (const op of t.toDelta()) s += typeof op.insert === 'string' ? op.insert : '\u0001';
    return s;
  };
  let placedInside = false;
  const pick = (s, lo, hi) => { // an index in [lo, hi]; "safe" histories never take one inside a pair
    for (;;) {
      const i = lo + ri(hi - lo + 1);
      const inside = i > 0 && i < s.length && hasPair(s[i - 1]) && /[\udc00-\udfff]/.test(s[i]);
      if (inside && !free) continue;
      if (inside) placedInside = true;
      return i;
    }
  };
  const svs = [];
  for (let round = 0; round < 4; ++round) {
    for (const d of docs) {
      const t = textOf(d);
      for (let k = 0; k < 5; ++k) {
        const s = unitsOf(t);
        const x = g();
        if (s.length >= 4 && x < 0.3) {
          const i = pick(s, 0, s.length - 1);
          let e = pick(s, i + 1, Math.min(s.length, i + 4));
          t.delete(i, e - i);
        } else if (fmt && s.length >= 2 && x < 0.45) {
          const i = pick(s, 0, s.length - 1);
          const e = pick(s, i + 1, Math.min(s.length, i + 6));
          t.format(i, e - i, { bold: g() < 0.6 ? true : null });
        } else if (fmt && x < 0.55) {
          t.insertEmbed(pick(s, 0, s.length), { img: 'i' + ri(100) });
        } else {
          let ins = '';
          for (let n = 1 + ri(5); n > 0; --n) ins += ALPHABET[ri(ALPHABET.length)];
          t.insert(pick(s, 0, s.length), ins);
        }
      }
    }
    // partial gossip: every replica pulls what it lacks from one random peer
    for (let i = 0; i < nrep; ++i) {
      const j = (i + 1 + ri(nrep - 1)) % nrep;
      const u = Y.encodeStateAsUpdate(docs[j], Y.encodeStateVector(docs[i]));
      updates.push(u);
      Y.applyUpdate(docs[i], u);
    }
    if (round < 3) svs.push(Y.encodeStateVector(docs[ri(nrep)]));
  }
  svs.push(Uint8Array.from([0]));
  for (const d of docs) updates.push(Y.encodeStateAsUpdate(d));
  const c = record('seed_' + seed, free ? 'free' : 'safe', updates, svs, { fmt, nested, replicas: nrep });
  c.pair_split = placedInside || c.has_fffd;
  return c;
}

// ---- hand-built updates
function vu(out, v) { while (v > 127) { out.push(128 | (v % 128)); v = Math.floor(v / 128); } out.push(v); }
function str(out, s) { const b = Buffer.from(s, 'utf8'); vu(out, b.length); for (const x of b) out.push(x); }
// a ContentString item: {origin, right: [client, clock]} or {root, sub}
function sitem(s, o) {
  const out = [4 | (o.origin ? 0x80 : 0) | (o.right ? 0x40 : 0) | (o.sub !== undefined ? 0x20 : 0)];
  if (o.origin) { vu(out, o.origin[0]); vu(out, o.origin[1]); }
  if (o.right) { vu(out, o.right[0]); vu(out, o.right[1]); }
  if (!o.origin && !o.right) { out.push(1); str(out, o.root); if (o.sub !== undefined) str(out, o.sub); }
  str(out, s);
  return out;
}
// sections: [[client, clock, [struct bytes...]]], ds: [[client, [[clock, len]...]]]
function upd(sections, ds) {
  const out = [];
  vu(out, sections.length);
  for (const [client, clock, structs] of sections) {
    vu(out, structs.length); vu(out, client); vu(out, clock);
    for (const s of structs) for (const x of s) out.push(x);
  }
  vu(out, (ds || []).length);
  for (const [client, ranges] of ds || []) {
    vu(out, client); vu(out, ranges.length);
    for (const [c, l] of ranges) { vu(out, c); vu(out, l); }
  }
  return Uint8Array.from(out);
}
function sv(entries) {
  const out = [];
  vu(out, entries.length);
  for (const [c, k] of entries) { vu(out, c); vu(out, k); }
  return Uint8Array.from(out);
}
const cutSvs = (client, n) => { const r = [sv([])]; for (let k = 1; k < n; ++k) r.push(sv([[client, k]])); return r; };

function handBuilt() {
  const out = [];
  const add = (name, updates, svs, split, note) => {
    const c = record(name, 'hand', updates, svs, { note });
    c.pair_split = split;
    out.push(c);
  };
  const whole = upd([[5, 0, [sitem('a😀b', { root: 't' })]]]);  // units a0 😀1,2 b3
  // a partly known duplicate: the first units arrive first (or last), the author's struct is cut
  const part2 = upd([[5, 0, [sitem('ax', { root: 't' })]]]);
  const part3 = upd([[5, 0, [sitem('axy', { root: 't' })]]]);
  const part1 = upd([[5, 0, [sitem('a', { root: 't' })]]]);
  add('overlap_inside', [part2, whole], cutSvs(5, 4), true, 'units [0,2) then [0,4): the cut at 2 is inside the pair');
  add('overlap_inside_rev', [whole, part2], cutSvs(5, 4), true, 'the same two updates, the whole struct first');
  add('overlap_boundary_3', [part3, whole], cutSvs(5, 4), false, 'units [0,3) then [0,4): the cut at 3 is behind the pair');
  add('overlap_boundary_1', [part1, whole], cutSvs(5, 4), false, 'units [0,1) then [0,4): the cut at 1 is before the pair');
  add('overlap_boundary_1_rev', [whole, part1], cutSvs(5, 4), false, 'the same, the whole struct first');
  // delete-set ranges over the pair
  add('ds_inside', [upd([[5, 0, [sitem('a😀b', { root: 't' })]]], [[5, [[1, 1]]]])], cutSvs(5, 4), true,
      'range [1,1] ends inside the pair: a deleted half and a live U+FFFD');
  add('ds_inside_late', [whole, upd([], [[5, [[2, 1]]]])], cutSvs(5, 4), true, 'range [2,1] begins inside the pair, in an update of its own');
  add('ds_whole', [upd([[5, 0, [sitem('a😀b', { root: 't' })]]], [[5, [[1, 2]]]])], cutSvs(5, 4), false, 'range [1,2] covers the pair');
  // one client's three consecutive inserts as three deltas; the engine glues them, a peer's origin cuts the glue
  const g1 = upd([[5, 0, [sitem('ab', { root: 't' })]]]);             // a0 b1
  const g2 = upd([[5, 2, [sitem('😀c', { origin: [5, 1] })]]]);        // 😀2,3 c4
  const g3 = upd([[5, 5, [sitem('de', { origin: [5, 4] })]]]);        // d5 e6
  const peerIn = upd([[9, 0, [sitem('é𝄞', { origin: [5, 2], right: [5, 3] })]]]);
  const peerAt = upd([[9, 0, [sitem('é𝄞', { origin: [5, 3], right: [5, 4] })]]]);
  add('glued', [g1, g2, g3], cutSvs(5, 7), false, 'three deltas of one client, nothing cuts them');
  add('glued_cut_pair', [g1, g2, g3, peerIn], cutSvs(5, 7).concat([sv([[9, 1]]), sv([[9, 2], [5, 3]])]), true,
      'a peer inserts between the two units of the pair in the middle piece');
  add('glued_cut_pair_first', [peerIn, g3, g2, g1], [sv([])], true, 'the same, the peer and the last piece first (parked until the gap fills)');
  add('glued_cut', [g1, g2, g3, peerAt], cutSvs(5, 7).concat([sv([[9, 1]])]), false, 'a peer inserts behind the pair in the middle piece');
  // string values of map entries: Yjs keeps the last UNIT of the string
  add('map_empty', [upd([[5, 0, [sitem('', { root: 'm', sub: 'e' })]]])], [sv([])], false, 'an empty ContentString item under a key');
  add('map_one', [upd([[5, 0, [sitem('z', { root: 'm', sub: 'k' })]]])], [sv([])], false, 'a 1-unit string under a key');
  add('map_pair_last', [upd([[5, 0, [sitem('x😀', { root: 'm', sub: 'k' })]]])], cutSvs(5, 3), false, 'x😀 under a key: the last unit is the low surrogate');
  add('map_three', [upd([[5, 0, [sitem('é漢€', { root: 'm', sub: 'k' }), sitem('q', { root: 'm', sub: 'j' })]]])], cutSvs(5, 4), false,
      '2- and 3-byte characters under a key, a second key');
  return out;
}

// 10 000 x 😀é漢 (40 000 units, 90 KB); peers insert at 20 001 (inside a pair) and 20 002, a delete covers [39 990, 39 998)
function longString() {
  const a = newDoc(1);
  a.getText('t').insert(0, '😀é漢'.repeat(10000));
  const base = Y.encodeStateAsUpdate(a);
  const svA = Y.encodeStateVector(a);
  const peer = (client, f) => { const d = newDoc(client); Y.applyUpdate(d, base); f(d.getText('t')); return d; };
  const b = peer(2, (t) => t.insert(20001, 'X€'));
  const c = peer(3, (t) => t.insert(20002, 'Y𝄞'));
  const d = peer(4, (t) => t.delete(39990, 8));
  const updates = [base, Y.encodeStateAsUpdate(b), Y.encodeStateAsUpdate(c, svA), Y.encodeStateAsUpdate(d, svA)];
  const svs = [sv([]), sv([[1, 20000]]), sv([[1, 20002], [2, 1]]), sv([[1, 39992], [3, 3]]), sv([[1, 20001]]), sv([[1, 40000]])];
  const r = record('long_string', 'long', updates, svs, { note: '40 000 units in one struct, cut at 20 001, 20 002, 39 990 and 39 998' });
  r.pair_split = true;
  return r;
}

const histories = [];
for (let s = 0; s < NSEEDS; ++s) histories.push(randomHistory(s));
const hand = handBuilt();
const long = longString();

// the conditions the tests rely on
const must = (ok, what) => { if (!ok) throw new Error('fixture condition failed: ' + what); };
must(histories.filter((c) => c.pair_split).length >= 15, '>= 15 histories with a split pair');
must(histories.filter((c) => !c.pair_split).length >= 15, '>= 15 histories without');
must(histories.filter((c) => c.fmt).length >= 10, '>= 10 histories with format or embed');
for (const c of histories.concat([long])) {
  must(!c.apply_throws && !c.pending, c.name + ' applies with nothing pending');
  must(c.state === c.state_rev, c.name + ': forward canonical == reversed canonical');
  must(typeof c.merged === 'number', c.name + ': mergeUpdates answers');
}

const cat = Buffer.concat(blobs);
const outDir = process.argv[2] || path.join(__dirname, '..');
fs.writeFileSync(path.join(outDir, 'text.json'), JSON.stringify({
  generator: 'tests/golden/gen/gen_text_fixtures.js', yjs: '13.5.16', lib0: '0.2.42',
  histories, hand, long,
  blob_lens: blobs.map((b) => b.length),
  blobs_z: zlib.deflateSync(cat, { level: 9 }).toString('base64'),
}, null, 0) + '\n');
console.log('text.json:', histories.length, 'histories,', histories.filter((c) => c.pair_split).length, 'split,',
            histories.filter((c) => c.fmt).length, 'with format/embed,', histories.filter((c) => c.nested).length, 'under m.doc,',
            hand.length, 'hand-built,', blobs.length, 'blobs,', cat.length, 'bytes raw,', fs.statSync(path.join(outDir, 'text.json')).size, 'bytes');
