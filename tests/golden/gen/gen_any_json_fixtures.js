#!/usr/bin/env node
// lib0 `any` encodings with Node's JSON.stringify of the value Yjs reads from them (TEST
// INFRASTRUCTURE ONLY; runs against the in-image Yjs 13.5.16 + lib0 0.2.42 through load_yjs.js).
// Every value is hand-encoded here (so float32, -0, NaN payloads, undefined and nesting are exactly
// what the case says), wrapped in one YMap set on root 'users' (gen_anyform_fixtures.js's update
// shape), applied to a fresh Y.Doc and read back with getMap('users').get(key): that is lib0's
// readAny. tests/test_any_json_text.py holds yc_json.h's any_json_text to these texts.
//   json: JSON.stringify(value), or null when the value is undefined (`undef`) or a BigInt (`big`:
//         its decimal text; JSON.stringify throws on BigInt)
// Usage: node gen_any_json_fixtures.js <out_dir>  ->  <out_dir>/any_json.json
'use strict';
const fs = require('fs');
const path = require('path');
const { loadYjs } = require('./load_yjs.js');

const Y = loadYjs();

const vu = (n) => { const o = []; while (n > 127) { o.push(128 | (n & 127)); n = Math.floor(n / 128); } o.push(n); return o; };
const vi = (n, negZero = false) => {  // lib0 writeVarInt
  const neg = n < 0 || negZero;
  n = Math.abs(n);
  const o = [(n > 63 ? 128 : 0) | (neg ? 64 : 0) | (n & 63)];
  n = Math.floor(n / 64);
  while (n > 0) { o.push((n > 127 ? 128 : 0) | (n & 127)); n = Math.floor(n / 128); }
  return o;
};
const vs = (s) => { const b = Buffer.from(s, 'utf8'); return [...vu(b.length), ...b]; };
const f64 = (x) => { const b = Buffer.alloc(8); b.writeDoubleBE(x); return [123, ...b]; };
const f32 = (x) => { const b = Buffer.alloc(4); b.writeFloatBE(x); return [124, ...b]; };
const int = (n) => [125, ...vi(n)];
const str = (s) => [119, ...vs(s)];
const big = (n) => { const b = Buffer.alloc(8); b.writeBigInt64BE(n); return [122, ...b]; };
const bin = (a) => [116, ...vu(a.length), ...a];
const arr = (xs) => [117, ...vu(xs.length), ...xs.flat()];
const obj = (kv) => [118, ...vu(kv.length), ...kv.map(([k, v]) => [...vs(k), ...v]).flat()];
const UNDEF = [127], NULL = [126], TRUE = [120], FALSE = [121];

const nest = (levels, leaf, objects) => {
  let v = leaf;
  for (let i = 0; i < levels; ++i) v = objects && i % 2 ? obj([['n' + i, v]]) : arr([v]);
  return v;
};

const cases = [];
const add = (name, bytes) => cases.push([name, bytes]);

for (const n of [0, 1, -1, 63, 64, -63, -64, 8191, 8192, -8192, 1048575, 1048576, 134217727, 134217728, 2147483647, -2147483647])
  add('int_' + n, int(n));
add('int_neg_zero', [125, 0x40]);
add('f64_neg_zero', f64(-0));
add('f64_0.1+0.2', f64(0.1 + 0.2));
add('f64_1e21', f64(1e21));
add('f64_1e-7', f64(1e-7));
add('f64_5e-324', f64(5e-324));
add('f64_max', f64(Number.MAX_VALUE));
add('f64_2p53', f64(9007199254740992));
add('f64_123456789012345680000', f64(123456789012345680000));
add('f64_neg', f64(-1234.5678));
add('f32_1.1', f32(1.1));
add('f32_0.5', f32(0.5));
add('f32_nan', [124, 0x7f, 0xc0, 0, 0]);
add('f32_inf', f32(Infinity));
add('nan', f64(NaN));
add('inf', f64(Infinity));
add('ninf', f64(-Infinity));
add('null', NULL);
add('true', TRUE);
add('false', FALSE);
add('undef_top', UNDEF);
add('str_empty', str(''));
add('str_escapes', str('q"b\\s/ \b\f\n\r\t end'));
add('str_ctl', str('\u0001\u001f\u007f'));
add('str_utf8', str('é € \u{1F600}  '));
add('str_long', str('x'.repeat(300)));
add('obj_empty', obj([]));
add('arr_empty', arr([]));
add('obj_1', obj([['a', int(1)]]));
add('arr_1', arr([int(1)]));
add('obj_2', obj([['a', obj([['b', str('c')]])], ['z', arr([NULL, TRUE])]]));
add('arr_2', arr([arr([int(1), int(2)]), obj([['k', FALSE]])]));
add('arr_63', nest(63, int(7), false));
add('mixed_63', nest(63, str('leaf'), true));
add('arr_64', nest(64, int(7), false));
add('undef_in_obj', obj([['a', UNDEF], ['b', int(2)], ['c', UNDEF]]));
add('undef_only_obj', obj([['a', UNDEF]]));
add('undef_first_obj', obj([['a', UNDEF], ['b', UNDEF], ['c', int(3)]]));
add('undef_in_arr', arr([UNDEF, int(1), UNDEF]));
add('undef_nested', arr([obj([['u', UNDEF], ['v', arr([UNDEF])]])]));
add('key_escapes', obj([['k"\\\n\u0002', int(1)], ['é\u{1F600}', int(2)], ['', int(3)]]));
add('bin_0', bin([]));
add('bin_3', bin([0, 127, 255]));
add('bin_in_arr', arr([bin([1, 2]), bin([])]));
add('big_9', big(9n));
add('big_neg', big(-1234567890123456789n));
add('big_min', big(-9223372036854775808n));
add('big_max', big(9223372036854775807n));

// seeded values
let seed = 0x2545f491;
const rnd = (n) => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return Math.floor((seed / 4294967296) * n); };
const words = ['a', 'users', 'msg', 'kéy', 'line\nbreak', 'tab\t', '"q"', '\u{1F680}', 'name_longer_than_eight', ''];
const gen = (depth) => {
  const t = rnd(depth > 3 ? 9 : 12);
  switch (t) {
    case 0: return int(rnd(2) ? rnd(1 << 30) : -rnd(5000));
    case 1: return f64((rnd(2000001) - 1000000) / (1 + rnd(997)));
    case 2: return f64(Math.pow(10, rnd(60) - 30) * (1 + rnd(9999)));
    case 3: return f32((rnd(20001) - 10000) / 128);
    case 4: return str(words[rnd(words.length)] + (rnd(2) ? words[rnd(words.length)] : ''));
    case 5: return [NULL, TRUE, FALSE][rnd(3)];
    case 6: return UNDEF;
    case 7: return bin(Array.from({ length: rnd(5) }, () => rnd(256)));
    case 8: return int(rnd(128) - 64);
    case 9: case 10: return arr(Array.from({ length: rnd(5) }, () => gen(depth + 1)));
    default: {
      const n = rnd(5), kv = [];
      for (let i = 0; i < n; ++i) kv.push([String.fromCharCode(97 + i) + words[rnd(words.length)], gen(depth + 1)]);  // distinct, never an array index
      return obj(kv);
    }
  }
};
for (let i = 0; i < 160; ++i) add('seeded_' + i, gen(0));

const update = (value) => Uint8Array.from([1, 1, 77, 0, 0x28, 1, ...vs('users'), ...vs('k'), 1, ...value, 0]);
const out = [];
for (const [name, bytes] of cases) {
  const doc = new Y.Doc();
  Y.applyUpdate(doc, update(bytes));
  const v = doc.getMap('users').get('k');
  const c = { name, any: Buffer.from(bytes).toString('hex') };
  if (typeof v === 'bigint') { c.json = null; c.big = v.toString(); }
  else if (v === undefined) { c.json = null; c.undef = true; }
  else c.json = JSON.stringify(v);
  out.push(c);
}

const head = {
  note: 'lib0 any encodings (hex) with JSON.stringify of the value Yjs 13.5.16 / lib0 0.2.42 reads; see gen_any_json_fixtures.js',
  // nested one level past the writer's 64-level stack: refused, not written
  too_deep: Buffer.from(nest(65, int(7), false)).toString('hex'),
  // every strict prefix of these must be refused without a read past its end
  truncate: ['mixed_63', 'obj_2', 'str_utf8'],
};
const dir = process.argv[2] || '.';
const text = JSON.stringify(head).slice(0, -1) + ',"cases":[\n' + out.map((c) => JSON.stringify(c)).join(',\n') + '\n]}\n';
fs.writeFileSync(path.join(dir, 'any_json.json'), text);
console.log(`${out.length} cases`);
