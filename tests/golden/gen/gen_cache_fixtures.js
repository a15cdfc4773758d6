#!/usr/bin/env node
// Cache-refresh fixture generator (TEST INFRASTRUCTURE ONLY; runs in the build container, never on
// the GPU box). Drives the in-image Yjs 13.5.16 (see load_yjs.js) through small documents that keep
// an index map of their roots, the way crdt.js does, and records for each what crdt.js's open /
// refresh loop makes of it: the index as JSON and the cache object `c`,
//   for every [key, val] of Object.entries(ix.toJSON()): c[key] = (val == 'map' ? getMap(key) : getArray(key)).toJSON()
// run here in JavaScript on a fresh Y.Doc that applied the recorded updates.
//
// Per case: name, index (the index root's name), updates (hex), ix (JSON: undefined values are
// dropped by JSON.stringify), ix_keys (Object.keys of the index, so undefined entries are listed),
// c, and per index entry its name, JSON.stringify(name), Array.isArray(c[name]), and the winning
// item's content: its ref number and the bytes Item content writes (hex).
//
// Usage: node gen_cache_fixtures.js <out_dir>   → <out_dir>/cache.json
'use strict';
const fs = require('fs');
const path = require('path');
const { loadYjs } = require('./load_yjs.js');

const Y = loadYjs();
const hex = (u) => Buffer.from(u).toString('hex');

function mulberry32(a) {
  return function () {
    a |= 0; a = (a + 0x6D2B79F5) | 0;
    let t = Math.imul(a ^ (a >>> 15), 1 | a);
    t = (t + Math.imul(t ^ (t >>> 7), 61 | t)) ^ t;
    return ((t ^ (t >>> 14)) >>> 0) / 4294967296;
  };
}

function newDoc(client) {
  const d = new Y.Doc();
  d.clientID = client;
  return d;
}

function contentOf(item) { // ref and written bytes of an item's content
  const ref = item.content.getRef();
  if (ref === 7) return { ref, content: '01' }; // ContentType: the type ref of a Y.Map
  if (ref !== 8 && ref !== 3) throw new Error('unexpected content ref ' + ref);
  // ContentAny, ContentBinary: what Yjs writes for the same value as the only struct of a fresh document, cut out
  // of that update: 01 01 | client 01 | clock 00 | info | 01 01 'm' | 01 'k' | content | 00
  const tmp = newDoc(1);
  const vals = item.content.getContent();
  tmp.getMap('m').set('k', vals[vals.length - 1]);
  const u = Y.encodeStateAsUpdate(tmp);
  if (hex(u.slice(0, 4)) !== '01010100' || u[4] !== (0x20 | ref) || hex(u.slice(5, 10)) !== '01016d' + '016b' || u[u.length - 1] !== 0) throw new Error('update layout');
  return { ref, content: hex(u.slice(10, u.length - 1)) };
}

const cases = [];
// build(replica(client) -> Y.Doc) fills replicas; the case's updates are every replica's full state
function add(name, build, index) {
  index = index === undefined ? 'ix' : index;
  const reps = [];
  const replica = (client) => { const d = newDoc(client); reps.push(d); return d; };
  build(replica);
  const updates = reps.map((d) => Y.encodeStateAsUpdate(d));
  const doc = newDoc(999999);
  for (const u of updates) Y.applyUpdate(doc, u);
  // the loop of crdt.js, restated
  const h = {};
  h.ix = doc.getMap(index);
  const ix = h.ix.toJSON();
  const c = {};
  for (const [key, val] of Object.entries(ix)) {
    if (val == 'map') h[key] = doc.getMap(key); // eslint-disable-line eqeqeq
    else h[key] = doc.getArray(key);
    c[key] = h[key].toJSON();
  }
  const entries = Object.keys(ix).map((key) => Object.assign(
    { name: key, name_json: JSON.stringify(key), is_array: Array.isArray(c[key]) }, contentOf(h.ix._map.get(key))));
  cases.push({ name, index, updates: updates.map(hex), ix, ix_keys: Object.keys(ix), c, entries });
}

// a root that holds map entries AND list items (two replicas wrote it as different types): the
// kind the index asks for decides what toJSON shows
function both(replica, root, base) {
  replica(base).getMap(root).set('k', root);
  replica(base + 1).getArray(root).push([root, 1]);
}

add('empty', (r) => { r(1); });
add('no_index', (r) => { const d = r(1); d.getMap('users').set('a', 1); d.getArray('log').push([1, 2]); });
add('basic', (r) => {
  const d = r(1);
  d.getMap('ix').set('users', 'map');
  d.getMap('ix').set('log', 'array');
  d.getMap('users').set('alice', { age: 30, tags: ['a', 'b'] });
  d.getMap('users').set('bob', null);
  d.getArray('log').push(['x', 2, true, { y: [1.5] }]);
});
add('array_per_key', (r) => { // a map holding a Y.Array per key
  const d = r(2);
  d.getMap('ix').set('rooms', 'map');
  for (const k of ['lobby', 'den', 'attic']) {
    const a = new Y.Array();
    d.getMap('rooms').set(k, a);
    a.push([k + '1', k + '2']);
  }
  d.getMap('rooms').get('den').delete(0, 1);
});
add('readded', (r) => {
  const d = r(3);
  const ix = d.getMap('ix');
  ix.set('a', 'map'); ix.delete('a'); ix.set('a', 'array');
  ix.set('b', 'map'); ix.delete('b');
  ix.set('c', 'array'); ix.set('c', 'map');
  d.getArray('a').push([1]);
  d.getMap('b').set('gone', 1);
  d.getMap('c').set('here', 'yes');
});
add('all_deleted', (r) => {
  const d = r(4);
  d.getMap('ix').set('a', 'map'); d.getMap('ix').delete('a');
  d.getMap('a').set('k', 1);
});
add('ghost_roots', (r) => {
  const d = r(5);
  d.getMap('ix').set('ghost', 'map'); d.getMap('ix').set('ghost2', 'array');
  d.getMap('real').set('k', 1);
});
add('wrong_kind', (r) => {
  const d = r(6);
  d.getMap('ix').set('list', 'map'); d.getMap('ix').set('dict', 'array');
  d.getArray('list').push([1, 2, 3]);
  d.getMap('dict').set('k', 'v');
});
{
  const values = [
    ['v_map', 'map'], ['v_array', 'array'], ['v_Map', 'Map'], ['v_1', 1], ['v_null', null], ['v_undef', undefined],
    ['v_amap', ['map']], ['v_aamap', [['map']]], ['v_obj', {}], ['v_aaamap', [[['map']]]], ['v_aMap', ['Map']],
    ['v_a2', ['map', 'map']], ['v_aempty', []], ['v_a1', [1]], ['v_anull', [null]], ['v_maps', 'map '], ['v_empty', ''],
    ['v_bytes', new Uint8Array([109, 97, 112])], ['v_objmap', { map: 'map' }], ['v_0', 0], ['v_false', false],
    ['v_true', true], ['v_f', 1.5], ['v_aobj', [{}]], ['v_m', 'm'],
  ];
  for (let part = 0; part < 3; ++part) {
    add('values_' + part, (r) => {
      const d = r(10);
      let base = 20;
      values.forEach(([name, val], i) => {
        if (i % 3 !== part) return;
        d.getMap('ix').set(name, val);
        both(r, name, base);
        base += 2;
      });
      if (part === 0) { // a shared type stored in the index
        const m = new Y.Map();
        d.getMap('ix').set('v_ymap', m);
        m.set('map', 'map');
        both(r, 'v_ymap', base);
      }
    });
  }
}
add('lists_itself', (r) => {
  const d = r(7);
  d.getMap('ix').set('ix', 'map'); d.getMap('ix').set('m', 'map');
  d.getMap('m').set('k', [1, 2]);
});
add('escaped_names', (r) => {
  const d = r(8);
  for (const n of ['"', '\\', '\u0001', '\u2028', '\u{1F600}', 'a"b\\c\n', '\u00e9t\u00e9', '\u001f\t']) {
    d.getMap('ix').set(n, 'map');
    d.getMap(n).set(n, n);
  }
});
add('empty_name', (r) => {
  const d = r(9);
  d.getMap('ix').set('', 'array'); d.getMap('ix').set('x', 'map');
  d.getArray('').push(['nameless']);
  d.getMap('x').set('', 'empty key');
});
add('integer_names', (r) => {
  const d = r(11);
  for (const n of ['10', '9', '1', '01', '100']) { d.getMap('ix').set(n, 'array'); d.getArray(n).push([n]); }
});
add('prefix_names', (r) => {
  const d = r(12);
  for (const n of ['ab', 'a', 'abc', 'b', 'aB', 'a ']) { d.getMap('ix').set(n, 'map'); d.getMap(n).set('n', n); }
});
add('name_64', (r) => {
  const d = r(13);
  const n = 'n'.repeat(64);
  d.getMap('ix').set(n, 'map'); d.getMap('ix').set('z', 'array');
  d.getMap(n).set('k', 64); d.getArray('z').push([1]);
});
add('name_65', (r) => {
  const d = r(14);
  const n = 'n'.repeat(65);
  d.getMap('ix').set(n, 'map'); d.getMap('ix').set('z', 'array');
  d.getMap(n).set('k', 65); d.getArray('z').push([1]);
});
add('other_index', (r) => {
  const d = r(15);
  d.getMap('index').set('users', 'map'); d.getMap('index').set('log', 'array');
  d.getMap('ix').set('decoy', 'map');
  d.getMap('users').set('u', 1); d.getArray('log').push([2]); d.getMap('decoy').set('d', 3);
}, 'index');
add('concurrent_low_wins', (r) => {
  const a = r(100); const b = r(200);
  a.getMap('ix').set('r', 'map'); b.getMap('ix').set('r', 'array');
  both(r, 'r', 300);
});
add('concurrent_high_wins', (r) => {
  const a = r(100); const b = r(200);
  a.getMap('ix').set('r', 'array'); b.getMap('ix').set('r', 'map');
  both(r, 'r', 300);
});
add('concurrent_three', (r) => {
  const a = r(100); const b = r(200); const c = r(50);
  a.getMap('ix').set('r', 'array'); a.getMap('ix').set('r', 'map');
  b.getMap('ix').set('r', ['map']); c.getMap('ix').set('r', 1); c.getMap('ix').delete('r'); c.getMap('ix').set('q', 'map');
  both(r, 'r', 300); both(r, 'q', 310);
});
add('text_root', (r) => {
  const d = r(16);
  d.getMap('ix').set('t', 'array');
  d.getText('t').insert(0, 'héllo "w"');
});
add('nested_levels', (r) => {
  const d = r(17);
  d.getMap('ix').set('tree', 'map'); d.getMap('ix').set('list', 'array');
  const l1 = new Y.Map(); d.getMap('tree').set('l1', l1);
  const l2 = new Y.Array(); l1.set('l2', l2);
  const l3 = new Y.Map(); l2.push([1, l3, 'x']);
  l3.set('leaf', { deep: [1, [2, [3]]] });
  const t = new Y.Text(); l1.set('text', t); t.insert(0, 'abc');
  const a1 = new Y.Array(); d.getArray('list').push([a1, null]);
  a1.push([new Y.Map(), 2]);
  a1.get(0).set('k', undefined);
});
// seeded small documents: several roots of either kind, some listed, some not, edits and deletes
for (let seed = 1; seed <= 12; ++seed) {
  add('seeded_' + seed, (r) => {
    const rnd = mulberry32(seed * 7919);
    const pick = (n) => Math.floor(rnd() * n);
    const docs = [r(1000 + seed), r(2000 + seed)];
    const nroots = 1 + pick(5);
    for (let k = 0; k < nroots; ++k) {
      const d = docs[pick(2)];
      const name = 'r' + k;
      const isMap = pick(2) === 0;
      if (pick(6) !== 0) d.getMap('ix').set(name, isMap ? 'map' : ['array', 'list', 2, null][pick(4)]);
      const n = pick(6);
      for (let j = 0; j < n; ++j) {
        const v = [j, 'v' + j, { j }, [j, j + 1], null, 1e21 + j, -0.5][pick(7)];
        if (isMap) d.getMap(name).set('k' + pick(4), v);
        else d.getArray(name).insert(pick(d.getArray(name).length + 1), [v]);
      }
      if (n && pick(3) === 0) {
        if (isMap) d.getMap(name).delete('k' + pick(4));
        else d.getArray(name).delete(pick(d.getArray(name).length), 1);
      }
      if (pick(5) === 0) d.getMap('ix').delete(name);
      if (isMap && pick(3) === 0) { const a = new Y.Array(); d.getMap(name).set('arr', a); a.push([seed, k]); }
    }
  });
}

const outDir = process.argv[2];
if (!outDir) { console.error('usage: gen_cache_fixtures.js <out_dir>'); process.exit(2); }
const text = JSON.stringify({ yjs: '13.5.16', cases }) + '\n';
fs.writeFileSync(path.join(outDir, 'cache.json'), text);
console.log(cases.length + ' cases, ' + text.length + ' bytes');
