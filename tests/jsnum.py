"""An independent reference for the JSON text of numbers and parsed JSON values, and the number
inputs the value-writer tests share (test_jsnum_reference.py pins it to Node's recorded texts,
test_num_text.py runs the host build against it, test_gpu_json_values.py the device build).

js_number_text is Number::toString (radix 10) as JSON.stringify writes it: the shortest round-trip
digits come from Python's repr(float) (David Gay's dtoa, nothing of yc_num.h), laid out by
ECMA-262's rules. The reading direction is float(text), correctly rounded for any digit count.
"""
import math
import random
import struct

SEED = 20240611
N_DOUBLES = 14000
N_F32_RANDOM = 2048
N_DEC_SEEDED = 300


# ---------------------------------------------------------------- the reference
def js_number_text(x: float) -> str:
    if math.isnan(x) or math.isinf(x):
        return "null"
    if x == 0:
        return "0"
    r = repr(abs(x))  # shortest digits: "123.45", "1e-07", "1.5e+300"
    mant, _, exp = r.partition("e")
    ip, _, fp = mant.partition(".")
    digits = (ip + fp).lstrip("0")
    n = len(ip) + (int(exp) if exp else 0)  # 0.d1d2... x 10^n, once the leading zeros are gone
    n -= len(ip + fp) - len(digits)
    digits = digits.rstrip("0")
    k = len(digits)
    assert 1 <= k <= 17
    if k <= n <= 21:
        t = digits + "0" * (n - k)
    elif 0 < n <= 21:
        t = digits[:n] + "." + digits[n:]
    elif -6 < n <= 0:
        t = "0." + "0" * (-n) + digits
    else:
        e = n - 1
        t = digits[0] + ("." + digits[1:] if k > 1 else "") + "e" + ("-" if e < 0 else "+") + str(abs(e))
    return ("-" if x < 0 else "") + t


_ESC = {'"': '\\"', "\\": "\\\\", "\b": "\\b", "\f": "\\f", "\n": "\\n", "\r": "\\r", "\t": "\\t"}


def js_string_text(s: str) -> str:
    out = ['"']
    for ch in s:
        c = ord(ch)
        if ch in _ESC:
            out.append(_ESC[ch])
        elif c < 0x20 or 0xD800 <= c <= 0xDFFF:  # controls, and a lone surrogate (well-formed JSON.stringify)
            out.append("\\u%04x" % c)
        else:
            out.append(ch)
    out.append('"')
    return "".join(out)


def js_stringify(value) -> str:
    """JSON.stringify of a value json.loads returned (dicts keep their order). Iterative: the
    fixtures nest deeper than Python recurses."""
    out = []
    stack = [value]  # values, and the literal texts between them
    lit = object()
    while stack:
        v = stack.pop()
        if isinstance(v, tuple) and v and v[0] is lit:
            out.append(v[1])
        elif v is None:
            out.append("null")
        elif v is True:
            out.append("true")
        elif v is False:
            out.append("false")
        elif isinstance(v, (int, float)):
            try:
                out.append(js_number_text(float(v)))
            except OverflowError:  # an integer text past MAX_VALUE: JSON.parse gives Infinity
                out.append("null")
        elif isinstance(v, str):
            out.append(js_string_text(v))
        elif isinstance(v, list):
            out.append("[")
            stack.append((lit, "]"))
            for i in range(len(v) - 1, -1, -1):
                stack.append(v[i])
                if i:
                    stack.append((lit, ","))
        elif isinstance(v, dict):
            out.append("{")
            stack.append((lit, "}"))
            items = list(v.items())
            for i in range(len(items) - 1, -1, -1):
                stack.append(items[i][1])
                stack.append((lit, ("," if i else "") + js_string_text(items[i][0]) + ":"))
        else:
            raise TypeError(type(v))
    return "".join(out)


# ---------------------------------------------------------------- bit patterns
def f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def f64_from(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def f32_from(bits: int) -> float:
    return struct.unpack("<f", struct.pack("<I", bits))[0]


_F64_INF, _F32_INF = 0x7FF0000000000000, 0x7F800000
_SIGN64, _SIGN32 = 1 << 63, 1 << 31

# (name, value): the values whose neighbourhoods the double list names
NAMED_DOUBLES = (
    ("1e21", 1e21), ("1e-6", 1e-6), ("1e-7", 1e-7), ("999999999999999900000", 999999999999999900000.0),
    ("123456789012345680000", 123456789012345680000.0), ("2^53", 2.0 ** 53), ("2^53-2", 2.0 ** 53 - 2), ("2^53+2", 2.0 ** 53 + 2),
    ("0.1+0.2", 0.1 + 0.2), ("MAX_VALUE", 1.7976931348623157e308), ("least normal", 2.2250738585072014e-308), ("1e22", 1e22),
    ("1e23", 1e23),
)


def _with_neighbours(bits):
    return [b for b in (bits, bits - 1, bits + 1) if 0 <= b < _F64_INF]


def double_bits():
    """The double list: bit patterns of finite doubles, sign bit included. Fixed by SEED."""
    out = []
    for e in range(-1074, 1024):  # lower_closer, the subnormal / normal seam
        out += _with_neighbours(f64_bits(math.ldexp(1.0, e)))
    for k in range(-323, 309):  # the decimal exponent estimate and its two corrections
        out += _with_neighbours(f64_bits(float("1e%d" % k)))
    out += range(1, 65)
    for _, x in NAMED_DOUBLES:
        out += _with_neighbours(f64_bits(x))
    out = list(dict.fromkeys(out))
    rng = random.Random(SEED)
    seen = set(out)
    while len(out) < N_DOUBLES:
        b = rng.getrandbits(63)
        if b < _F64_INF and b not in seen:
            seen.add(b)
            out.append(b)
    sign = random.Random(SEED + 1)
    return [b | _SIGN64 if sign.random() < 0.25 else b for b in out]


def float32_bits():
    """The float32 list: bit patterns of finite float32 values, sign bit included."""
    out = []
    for e in range(-149, 128):
        b = struct.unpack("<I", struct.pack("<f", math.ldexp(1.0, e)))[0]
        out += [v for v in (b, b - 1, b + 1) if 0 <= v < _F32_INF]
    out = list(dict.fromkeys(out))
    rng = random.Random(SEED + 2)
    seen = set(out)
    n = len(out) + N_F32_RANDOM
    while len(out) < n:
        b = rng.getrandbits(31)
        if b < _F32_INF and b not in seen:
            seen.add(b)
            out.append(b)
    sign = random.Random(SEED + 3)
    return [b | _SIGN32 if sign.random() < 0.25 else b for b in out]


# ---------------------------------------------------------------- decimal texts
def _split(bits):
    """a finite double >= 0 as m * 2^q"""
    be, m = (bits >> 52) & 0x7FF, bits & ((1 << 52) - 1)
    return (m | (1 << 52), be - 1075) if be else (m, -1074)


def _scaled_text(num: int, q: int, below: int = 0) -> str:
    """The exact decimal expansion of num * 2^q, minus `below` units of its last digit."""
    if q >= 0:
        return str((num << q) - below)
    s = str(num * 5 ** (-q) - below).rjust(-q + 1, "0")  # num * 2^q = num * 5^-q / 10^-q
    return s[:q] + "." + s[q:]


def midpoint_text(bits: int, below: int = 0) -> str:
    """The exact midpoint between the double `bits` (>= 0) and the next one up."""
    m, q = _split(bits)
    return _scaled_text(2 * m + 1, q - 1, below)


def _sticky(text: str) -> str:
    return (text if "." in text else text + ".") + "0" * 900 + "1"


def decimal_texts():
    """Number texts outside Number::toString's form (each takes the rewrite path): ties, ties with a
    sticky digit past the 800 that decide, one step below a tie, long and upper-case forms, and
    the overflow and underflow edges. The expected text of each is js_number_text(float(text))."""
    bits = double_bits()
    rng = random.Random(SEED + 4)
    picked = rng.sample(bits, N_DEC_SEEDED)
    max_bits = _F64_INF - 1
    picked += [1, 2, f64_bits(2.2250738585072014e-308), f64_bits(2.2250738585072014e-308) - 1, f64_bits(1.0), f64_bits(2.0 ** 53), max_bits - 1]
    out = []
    for b in picked:
        sign, mag = ("-" if b & _SIGN64 else ""), b & ~_SIGN64
        x = f64_from(b)
        mid = midpoint_text(mag)
        out += [sign + mid, sign + _sticky(mid), sign + midpoint_text(mag, below=1), "%.25e" % x, ("%.20e" % x).upper()]
    top = (2 ** 54 - 1) << 970  # halfway from MAX_VALUE to 2^1024
    out += ["1.7976931348623158e308", str(top), str(top - 1), "2.4703282292062327e-324", "2.4703282292062328e-324"]
    half_least = _scaled_text(1, -1075)
    out += [half_least, _sticky(half_least), _scaled_text(3, -1075), "0." + "0" * 400 + "1", "1" + "0" * 400]
    out += ["0e99999999999", "1e-99999999999", "1e99999999999"]
    return out


def decimal_expected(text: str) -> str:
    return js_number_text(float(text))
