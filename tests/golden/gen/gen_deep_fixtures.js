#!/usr/bin/env node
// Deep nested-type fixture generator (TEST INFRASTRUCTURE ONLY; runs in the build container, never
// on the GPU box). Drives the in-image Yjs 13.5.16 (see load_yjs.js) through histories whose types
// sit up to five levels below a root: types inside YArrays, types inside nested types, deletes and
// overwrites that kill whole subtrees, inserts into containers another replica already deleted,
// full states that carry GC structs where other inputs carry live items.
//
// Yjs's own bytes depend on the order of applyUpdate here (it only re-merges the GC structs a
// transaction touched), so every case records the forward AND the reversed apply; nothing aborts
// on a difference. Per case: updates, state / state_rev (13.6 canonical client order), the pending
// flags of either order (`flags` names the ones that are set), sv, toJSON of both roots, diffs, Y.mergeUpdates and a census
// of what the history contains. The parked cases add gen_pending_fixtures.js's per-step records
// for non-causal orders, where a child arrives before the type item that is its parent.
//
// The file stays small: the inputs (updates, requested state vectors) are kept once each in `blobs`,
// every distinct toJSON value once in `jsons`, and the records hold indices into them. Both tables
// are written deflated (zlib, level 9) and base64: `blobs_z` is the byte strings back to back, cut
// by `blob_lens`; `jsons_z` is the JSON text of the list of values.
// What Yjs answered in bytes is recorded as a digest, the first 16 hex digits of its SHA-256: a
// string where the bytes are already in the order-free form (v1.js coalesceGc leaves them as they
// are), else [digest of the bytes, digest of their coalesced form]. tests/deep_fixture.py reads it.
//
// Usage: node gen_deep_fixtures.js <out_dir>   → <out_dir>/deep.json
'use strict';
const fs = require('fs');
const path = require('path');
const { loadYjs } = require('./load_yjs.js');
const crypto = require('crypto');
const zlib = require('zlib');
const { canonicalUpdate, canonicalSv, coalesceGc, updateStats } = require('./v1.js');

const Y = loadYjs();
const ROOTS = { tree: 'map', list: 'array' };
const N_SEEDS = 60;
const N_PARKED = 12;

const blobs = []; const jsons = [];
const blobIndex = new Map(); const jsonIndex = new Map();
function intern(list, index, text) {
  if (!index.has(text)) { index.set(text, list.length); list.push(text); }
  return index.get(text);
}
const ref = (u) => intern(blobs, blobIndex, Buffer.from(u).toString('hex')); // the index of a byte string
const sha = (u) => crypto.createHash('sha256').update(u).digest('hex').slice(0, 16);
function dig(u) { // the digest record of an update
  const h = sha(u); const c = sha(coalesceGc(u));
  return h === c ? h : [h, c];
}
function jsonOf(m) {
  const json = {};
  for (const [rname, kind] of Object.entries(ROOTS)) json[rname] = kind === 'map' ? m.getMap(rname).toJSON() : m.getArray(rname).toJSON();
  return intern(jsons, jsonIndex, JSON.stringify(json));
}

function mulberry32(a) {
  return function () {
    a |= 0; a = (a + 0x6D2B79F5) | 0;
    let t = Math.imul(a ^ (a >>> 15), 1 | a);
    t = (t + Math.imul(t ^ (t >>> 7), 61 | t)) ^ t;
    return ((t ^ (t >>> 14)) >>> 0) / 4294967296;
  };
}
function makeRng(seed) {
  const r = mulberry32(seed);
  const int = (n) => Math.floor(r() * n);
  const pick = (a) => a[int(a.length)];
  return { r, int, pick };
}
function randClient(g, i) { // 1..5-byte varuints, as gen_fixtures.js
  const styles = [() => i + 1, () => 100 + i * 37, () => 20000 + g.int(1 << 20), () => ((i + 1) * 2654435761) >>> 0, () => (g.int(2 ** 31) + 1) >>> 0];
  return g.pick(styles)();
}
function newDoc(client) { const d = new Y.Doc(); d.clientID = client; return d; }
function scalar(g) {
  const k = g.int(5);
  if (k === 0) return g.int(100);
  if (k === 1) return 's' + g.int(1000);
  if (k === 2) return g.pick([true, false, null]);
  if (k === 3) return { n: g.int(50) };
  return 'ü😀' + g.int(9);
}
function shuffle(g, a) {
  const b = a.slice();
  for (let i = b.length - 1; i > 0; i--) { const j = g.int(i + 1); [b[i], b[j]] = [b[j], b[i]]; }
  return b;
}

// ---------------------------------------------------------------- walking a doc's types
const typeOf = (it) => (!it.deleted && it.content.type ? it.content.type : null);
function liveKids(t) {
  const kids = [];
  if (t instanceof Y.Map) t._map.forEach((it) => { if (typeOf(it)) kids.push(typeOf(it)); });
  else for (let it = t._start; it !== null; it = it.right) if (typeOf(it)) kids.push(typeOf(it));
  return kids;
}
// every live container with its depth below the root, by a walk from both roots
function containers(d) {
  const out = [];
  const walk = (t, depth) => { out.push({ t, depth }); for (const k of liveKids(t)) walk(k, depth + 1); };
  walk(d.getMap('tree'), 0); walk(d.getArray('list'), 0);
  return out;
}
// the deepest live type below each root, in levels
function rootDepth(d) {
  const under = (t) => liveKids(t).reduce((m, k) => Math.max(m, 1 + under(k)), 0);
  return { tree: under(d.getMap('tree')), list: under(d.getArray('list')) };
}
const idKey = (id) => id.client + ':' + id.clock;
// the live elements of a YArray, one entry per index: the item that holds it
function elements(arr) {
  const out = [];
  for (let it = arr._start; it !== null; it = it.right) if (!it.deleted && it.countable) for (let k = 0; k < it.length; k++) out.push(it);
  return out;
}

// ---------------------------------------------------------------- one recorded case
function applyAll(client, updates) {
  const m = newDoc(client);
  for (const u of updates) Y.applyUpdate(m, u);
  return m;
}
// the names of the flags that are set (every other one is false)
const flagsOf = (o) => Object.keys(o).filter((k) => o[k]);
const pendingOf = (m) => [m.store.pendingStructs !== null, m.store.pendingDs !== null];

function finishCase(name, updates, svs) {
  const m = applyAll(0x7ffffff0, updates);
  const rev = applyAll(0x7ffffff0, updates.slice().reverse());
  const diffs = [];
  for (const s of svs.slice(0, 3).concat([new Uint8Array([0])])) diffs.push([ref(s), dig(canonicalUpdate(Y.encodeStateAsUpdate(m, s)))]);
  let gcs = 0;
  for (const u of updates) gcs += updateStats(u).gcs;
  const depth = rootDepth(m);
  return {
    name,
    updates: updates.map(ref),
    state: dig(canonicalUpdate(Y.encodeStateAsUpdate(m))),
    state_rev: dig(canonicalUpdate(Y.encodeStateAsUpdate(rev))),
    flags: flagsOf({ pending: pendingOf(m)[0], pending_ds: pendingOf(m)[1], pending_rev: pendingOf(rev)[0], pending_ds_rev: pendingOf(rev)[1] }),
    sv: sha(canonicalSv(Y.encodeStateVector(m))),
    json: jsonOf(m),
    diffs,
    merged: sha(canonicalUpdate(Y.mergeUpdates(updates))),
    root_depth: depth,
    gc_in_input: gcs,
  };
}

// ---------------------------------------------------------------- random histories
function randomHistory(seed) {
  const g = makeRng(seed);
  const nRep = 2 + g.int(5);
  const rounds = 2 + g.int(4);
  const ops = 4 + g.int(9);
  const maxDepth = 2 + g.int(4);
  const docs = [];
  const used = new Set();
  for (let i = 0; i < nRep; i++) {
    let c; do { c = randClient(g, i); } while (used.has(c) || c === 0);
    used.add(c); docs.push(newDoc(c));
  }
  const census = { made_depth: 0, types_in_arrays: 0, subtree_deletes: 0, orphan_inserts: 0 };
  const killed = new Map(); // id of a type's item → the replica that deleted it
  const kill = (it, rep) => {
    if (!typeOf(it)) return;
    if (liveKids(typeOf(it)).length > 0) census.subtree_deletes++;
    if (!killed.has(idKey(it.id))) killed.set(idKey(it.id), rep);
  };
  // an insert into a container that another replica already deleted, itself or an ancestor
  const orphan = (t, rep) => {
    for (let it = t._item; it !== null; it = it.parent._item) {
      const k = killed.get(idKey(it.id));
      if (k !== undefined && k !== rep) return true;
    }
    return false;
  };
  const value = (c, inArray) => {
    if (c.depth < maxDepth && g.r() < 0.45) {
      census.made_depth = Math.max(census.made_depth, c.depth + 1);
      if (inArray) census.types_in_arrays++;
      return g.r() < 0.5 ? new Y.Map() : new Y.Array();
    }
    return scalar(g);
  };
  const log = []; // per-round deltas in causal order
  for (let rd = 0; rd < rounds; rd++) {
    docs.forEach((d, rep) => {
      const before = Y.encodeStateVector(d);
      for (let o = 0; o < ops; o++) {
        const c = g.pick(containers(d));
        if (c.t instanceof Y.Map) {
          const key = 'k' + g.int(3);
          const cur = c.t._map.get(key);
          if (g.r() < 0.75) {
            const v = value(c, false);
            if (cur) kill(cur, rep);
            if (orphan(c.t, rep)) census.orphan_inserts++;
            c.t.set(key, v);
          } else {
            if (cur) kill(cur, rep);
            c.t.delete(key);
          }
        } else {
          const el = elements(c.t);
          if (g.r() < 0.7 || el.length === 0) {
            const v = [value(c, true)];
            if (g.r() < 0.3) v.push(scalar(g));
            if (orphan(c.t, rep)) census.orphan_inserts++;
            c.t.insert(g.int(el.length + 1), v);
          } else {
            const p = g.int(el.length); const n = Math.min(el.length - p, 1 + g.int(3));
            for (const it of new Set(el.slice(p, p + n))) kill(it, rep);
            c.t.delete(p, n);
          }
        }
      }
      log.push(Y.encodeStateAsUpdate(d, before));
    });
    for (const d of docs) {
      if (g.r() < 0.6) {
        const p = g.pick(docs);
        if (p !== d) Y.applyUpdate(d, Y.encodeStateAsUpdate(p, Y.encodeStateVector(d)));
      }
    }
  }
  const full = docs.map((d) => Y.encodeStateAsUpdate(d));
  const svs = docs.map((d) => Y.encodeStateVector(d));
  const mixed = full.filter((_, i) => i % 2 === 0).concat(log.filter((_, i) => i % 3 !== 2));
  return {
    g, log, svs, census: Object.assign({ seed }, census),
    cases: [
      finishCase(`log_${seed}`, log, svs),
      finishCase(`full_${seed}`, full, svs),
      finishCase(`mixed_${seed}`, mixed, svs),
    ],
  };
}

// ---------------------------------------------------------------- hand-built histories
const delta = (d, sv) => Y.encodeStateAsUpdate(d, sv);
const sync = (to, from) => Y.applyUpdate(to, Y.encodeStateAsUpdate(from, Y.encodeStateVector(to)));

// root YMap `tree`, then n types below it, YArray and YMap in turn; the client of level i writes
// the child of the level-i container. With `cut`, one more client overwrites the top key while
// every level's writer, who has not seen that, inserts once more at its level. With `inList` the
// chain hangs below the root YArray `list` instead (YMap and YArray in turn), nothing deleted.
function chain(n, cut, inList = false) {
  const ups = [];
  const writers = [];
  const at = []; // per writer: its own handle of the container it wrote into
  let prev = null;
  for (let i = 0; i <= n; i++) {
    const d = newDoc(10 + i);
    if (prev) sync(d, prev);
    const sv = Y.encodeStateVector(d);
    let t = inList ? d.getArray('list') : d.getMap('tree');
    for (let k = 0; k < i; k++) t = t instanceof Y.Map ? t.get('c') : t.get(1);
    if (i === n) { if (t instanceof Y.Map) t.set('leaf', 'v' + i); else t.push(['v' + i]); } else {
      const child = t instanceof Y.Map ? new Y.Array() : new Y.Map();
      if (t instanceof Y.Map) { t.set('v', i); t.set('c', child); } else t.insert(0, [i, child]);
    }
    ups.push(delta(d, sv));
    writers.push(d); at.push(t); prev = d;
  }
  if (cut) {
    const x = newDoc(99);
    sync(x, prev);
    const sv = Y.encodeStateVector(x);
    x.getMap('tree').set('c', 'gone');
    ups.push(delta(x, sv));
    writers.forEach((d, i) => {
      const svw = Y.encodeStateVector(d);
      if (at[i] instanceof Y.Map) at[i].set('w', 'late' + i); else at[i].push(['late' + i]);
      ups.push(delta(d, svw));
    });
  }
  return finishCase(`chain_${inList ? 'list_' : ''}d${n}${cut ? '_cut' : ''}`, ups, writers.slice(0, 3).map((d) => Y.encodeStateVector(d)));
}

function rangeKillsTree() {
  const a = newDoc(1); const b = newDoc(2); const c = newDoc(3);
  const M = new Y.Map(); const A = new Y.Array();
  a.getArray('list').push(['v0', M, 'v1']); M.set('a', A); A.push([1, 2]);
  const ua = Y.encodeStateAsUpdate(a);
  Y.applyUpdate(b, ua); Y.applyUpdate(c, ua);
  const sv = Y.encodeStateVector(a);
  b.getArray('list').delete(0, 3);
  const Mc = c.getArray('list').get(1);
  Mc.get('a').push([3]); Mc.set('b', 'x');
  return finishCase('range_kills_tree', [ua, delta(b, sv), delta(c, sv)], [sv, Y.encodeStateVector(b), Y.encodeStateVector(c)]);
}

// 300 clients unshift one value each into the same empty depth-2 YArray: every item has a null
// origin and names the array's item as its parent, so the nested list has 300 roots
function manyRootsNested(dead) {
  const base = newDoc(1);
  const M = new Y.Map(); base.getMap('tree').set('m', M); M.set('arr', new Y.Array());
  const ub = Y.encodeStateAsUpdate(base); const sv = Y.encodeStateVector(base);
  const ups = [ub];
  for (let i = 0; i < 300; i++) {
    const d = newDoc(1000 + 3 * i);
    Y.applyUpdate(d, ub);
    d.getMap('tree').get('m').get('arr').unshift([i]);
    ups.push(delta(d, sv));
  }
  if (dead) {
    const x = newDoc(5);
    Y.applyUpdate(x, ub);
    x.getMap('tree').set('m', 0);
    ups.push(delta(x, sv));
  }
  return finishCase(`many_roots_nested_${dead ? 'dead' : 'live'}`, ups, [sv]);
}

// two clients set one key to a new type concurrently; a third saw only the loser and fills it
function rivalTypes() {
  const a = newDoc(1); const b = newDoc(2);
  a.getMap('tree').set('k', new Y.Map()); b.getMap('tree').set('k', new Y.Map());
  const ua = Y.encodeStateAsUpdate(a); const ub = Y.encodeStateAsUpdate(b);
  const both = applyAll(7, [ua, ub]);
  const loser = both.getMap('tree').get('k')._item.id.client === 1 ? b : a;
  const c = newDoc(3);
  Y.applyUpdate(c, Y.encodeStateAsUpdate(loser));
  const sv = Y.encodeStateVector(c);
  const arr = new Y.Array(); const inner = new Y.Map();
  c.getMap('tree').get('k').set('x', arr); arr.push([inner, 'tail']); inner.set('y', 1);
  return finishCase('rival_types', [ua, ub, delta(c, sv)], [Y.encodeStateVector(a), Y.encodeStateVector(b), Y.encodeStateVector(c)]);
}

// replica A deletes and garbage-collects a depth-2 type and sends its full state, where that type
// item is a GC struct; replica B, unaware, pushes into the (empty) type: its item names the type
// item as its parent id
function gcParent() {
  const a = newDoc(1); const b = newDoc(2);
  const M = new Y.Map(); a.getMap('tree').set('m', M); M.set('t', new Y.Array()); M.set('s', 1);
  Y.applyUpdate(b, Y.encodeStateAsUpdate(a));
  const sv = Y.encodeStateVector(b);
  a.getMap('tree').delete('m');
  b.getMap('tree').get('m').get('t').push([9]);
  const ua = Y.encodeStateAsUpdate(a);
  if (updateStats(ua).gcs === 0) throw new Error('gc_parent: the full state carries no GC struct');
  const ub = delta(b, sv);
  if (updateStats(ub).parents.length !== 1) throw new Error('gc_parent: the delta names no parent id');
  return finishCase('gc_parent', [ua, ub], [sv, Y.encodeStateVector(a)]);
}

function handBuilt() {
  const out = [];
  for (let n = 1; n <= 6; n++) { out.push(chain(n, false)); out.push(chain(n, true)); }
  for (let n = 4; n <= 6; n++) out.push(chain(n, false, true));
  out.push(rangeKillsTree(), manyRootsNested(false), manyRootsNested(true), rivalTypes(), gcParent());
  return out;
}

// ---------------------------------------------------------------- parked children
// applies `updates` one at a time to a fresh doc, a snapshot after every apply (the records of
// gen_pending_fixtures.js runCase). `parked` marks a step after which a received item is still
// waiting and the type item it names as its parent by id has not been integrated either.
function runCase(name, updates, svs, g) {
  const m = newDoc(0x7ffffff0);
  const steps = [];
  const named = [];
  let parkedSteps = 0;
  for (const u of updates) {
    Y.applyUpdate(m, u);
    named.push(...updateStats(u).parents);
    const st = Y.encodeStateAsUpdate(m);
    const tsv = svs[g.int(svs.length)];
    const parked =m.store.pendingStructs !== null &&
      named.some((p) => Y.getState(m.store, p.client) <= p.clock && Y.getState(m.store, p.parent[0]) <= p.parent[1]);
    if (parked) parkedSteps++;
    steps.push({
      state: dig(canonicalUpdate(st)), sv: sha(canonicalSv(Y.encodeStateVector(m))),
      flags: flagsOf({ pending: m.store.pendingStructs !== null, pending_ds: m.store.pendingDs !== null, parked }),
      delta: [ref(tsv), dig(canonicalUpdate(Y.encodeStateAsUpdate(m, tsv)))],
      json: jsonOf(m),
    });
  }
  return { name, updates: updates.map(ref), parked_steps: parkedSteps, steps };
}

const pack = (buf) => zlib.deflateSync(buf, { level: 9 }).toString('base64');

function main() {
  const outDir = process.argv[2] || path.join(__dirname, '..');
  const cases = handBuilt();
  const hist = [];
  for (let s = 1; s <= N_SEEDS; s++) { const h = randomHistory(7000 + s); h.seed = 7000 + s; hist.push(h); cases.push(...h.cases); }
  // the parked orders come from the shortest logs that still kill a subtree: every step is a record
  const short = hist.filter((h) => h.census.subtree_deletes > 0 && h.log.length > 3)
    .sort((a, b) => a.log.length - b.log.length || a.seed - b.seed).slice(0, N_PARKED);
  const parked = [];
  for (const h of short) {
    const svs = h.svs.concat([new Uint8Array([0])]);
    parked.push(runCase(`shuffled_${h.seed}`, shuffle(h.g, h.log), svs, h.g));
    parked.push(runCase(`reversed_${h.seed}`, h.log.slice().reverse(), svs, h.g));
    const drop = 1 + h.g.int(h.log.length - 1);
    parked.push(runCase(`lost_${h.seed}`, shuffle(h.g, h.log.filter((_, i) => i !== drop)), svs, h.g));
  }
  const f = path.join(outDir, 'deep.json');
  const doc = { generator: 'tests/golden/gen/gen_deep_fixtures.js', yjs: '13.5.16', lib0: '0.2.42', roots: ROOTS, histories: hist.map((h) => h.census), cases, parked, jsons_z: pack(Buffer.from('[' + jsons.join(',') + ']')), blob_lens: blobs.map((h) => h.length / 2), blobs_z: pack(Buffer.from(blobs.join(''), 'hex')) };
  // one record per line
  const text = Object.entries(doc).map(([k, v]) => (['histories', 'cases', 'parked'].includes(k)
    ? `"${k}":[\n${v.map((x) => JSON.stringify(x)).join(',\n')}\n]` : `"${k}":${JSON.stringify(v)}`)).join(',\n');
  fs.writeFileSync(f, `{\n${text}\n}\n`);
  const quiet = cases.filter((c) => c.flags.length === 0);
  const sum = (k) => hist.reduce((a, h) => a + h.census[k], 0);
  console.log(f, fs.statSync(f).size, 'bytes', cases.length, 'cases', quiet.length, 'nothing pending',
    quiet.filter((c) => String(c.state) !== String(c.state_rev)).length, 'order dependent', parked.length, 'parked cases',
    parked.reduce((a, c) => a + c.steps.length, 0), 'steps', parked.reduce((a, c) => a + c.parked_steps, 0), 'parked for a parent');
  console.log('subtree_deletes', sum('subtree_deletes'), 'orphan_inserts', sum('orphan_inserts'), 'types_in_arrays', sum('types_in_arrays'),
    'random live_depth>=4', cases.filter((c) => /^(log|full|mixed)_/.test(c.name) && Math.max(c.root_depth.tree, c.root_depth.list) >= 4).length,
    'live_depth>=5', cases.filter((c) => Math.max(c.root_depth.tree, c.root_depth.list) >= 5).length, 'gc in input', cases.filter((c) => c.gc_in_input > 0).length);
}

main();
