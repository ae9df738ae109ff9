"""An independent model of the header rules (hashlib and Python integers, no engine code): the block
hash, arith_uint256's SetCompact / GetCompact, CheckProofOfWork, CalculateNextWorkRequired,
GetMedianTimePast, the order of ContextualCheckBlockHeader's rules and GetBlockProof, written from
the rules of include/bcc_amd.h.  tests/golden/header_cases.json.gz pins it to recorded results of
the reference (test_headers_host.py)."""
import hashlib
import struct

OK, HIGH_HASH, PREV_MISMATCH, BAD_DIFFBITS, TIME_TOO_OLD, TIME_TOO_NEW, BAD_VERSION = range(7)
MASK = (1 << 256) - 1


def sha256d(b):
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()


def header(version, prev, merkle, time, bits, nonce):
    return struct.pack("<i32s32sIII", version, prev, merkle, time, bits, nonce)


def fields(h):
    """version (signed), prev, merkle, time, bits, nonce of an 80-byte header."""
    return struct.unpack("<i32s32sIII", h)


def set_compact(bits):
    """(target, negative, overflow) as arith_uint256::SetCompact gives them."""
    size, word = bits >> 24, bits & 0x007fffff
    if size <= 3:
        word >>= 8 * (3 - size)
        target = word
    else:
        target = (word << 8 * (size - 3)) & MASK
    negative = word != 0 and bits & 0x00800000 != 0
    overflow = word != 0 and (size > 34 or (word > 0xff and size > 33) or (word > 0xffff and size > 32))
    return target, negative, overflow


def get_compact(v):
    size = (v.bit_length() + 7) // 8
    c = (v << 8 * (3 - size)) if size <= 3 else (v >> 8 * (size - 3))
    c &= 0xffffffff
    if c & 0x00800000:
        c >>= 8
        size += 1
    return c | size << 24


def check_pow(hash32, bits, limit):
    target, negative, overflow = set_compact(bits)
    if negative or overflow or target == 0 or target > limit:
        return False
    return int.from_bytes(hash32, "little") <= target


def next_work(last_bits, last_time, first_time, timespan, limit, no_retargeting=False):
    """CalculateNextWorkRequired: the multiplier is truncated to 32 bits and the product to 256."""
    if no_retargeting:
        return last_bits
    span = min(max(last_time - first_time, timespan // 4), timespan * 4)
    v = (set_compact(last_bits)[0] * (span & 0xffffffff)) & MASK
    return get_compact(min(v // timespan, limit))


def block_proof(bits):
    target, negative, overflow = set_compact(bits)
    if negative or overflow or target == 0:
        return 0
    return (~target & MASK) // (target + 1) + 1


def check(headers, params, anchor=None, max_time=0):
    """bcc_headers_batch.  params: dict(pow_limit=int, timespan, spacing, no_retargeting, bip34,
    bip66, bip65); anchor: None or dict(height, hash, bits, times (newest first), period_first_time).
    Returns dict(first_invalid, status, hashes, chain_work)."""
    interval = params["timespan"] // params["spacing"]
    limit = params["pow_limit"]
    base = anchor["height"] + 1 if anchor else 0
    hashes = [sha256d(h) for h in headers]
    parsed = [fields(h) for h in headers]
    status = []
    for i, (version, prev, _, time, bits, _) in enumerate(parsed):
        status.append(OK)
        if not check_pow(hashes[i], bits, limit):
            status[i] = HIGH_HASH
            continue
        if anchor is None and i == 0:
            continue
        height = base + i
        if prev != (hashes[i - 1] if i else anchor["hash"]):
            status[i] = PREV_MISMATCH
            continue
        # the times before this header, newest first, as far back as they are known
        before = [parsed[k][3] for k in range(i - 1, -1, -1)] + (list(anchor["times"]) if anchor else [])
        prev_bits = parsed[i - 1][4] if i else anchor["bits"]
        want = prev_bits
        if height % interval == 0:
            first = parsed[i - interval][3] if i >= interval else anchor["period_first_time"]
            want = next_work(prev_bits, before[0], first, params["timespan"], limit,
                             params.get("no_retargeting", False))
        if bits != want:
            status[i] = BAD_DIFFBITS
            continue
        window = sorted(before[:11])
        if time <= window[len(window) // 2]:
            status[i] = TIME_TOO_OLD
        elif max_time != 0 and time > max_time:
            status[i] = TIME_TOO_NEW
        elif ((version < 2 and height >= params.get("bip34", 0)) or
              (version < 3 and height >= params.get("bip66", 0)) or
              (version < 4 and height >= params.get("bip65", 0))):
            status[i] = BAD_VERSION
    first_invalid = next((i for i, s in enumerate(status) if s != OK), len(headers))
    work = sum(block_proof(parsed[i][4]) for i in range(first_invalid)) & MASK
    return {"first_invalid": first_invalid, "status": status, "hashes": hashes, "chain_work": work}


def mine(version, prev, merkle, time, bits, limit=MASK, start=0):
    """A header whose hash meets bits (any nonce from `start` up); cheap at low difficulty."""
    head = struct.pack("<i32s32sII", version, prev, merkle, time, bits)
    for nonce in range(start, 1 << 32):
        h = head + struct.pack("<I", nonce)
        if check_pow(sha256d(h), bits, limit):
            return h
    raise ValueError("no nonce")


def unmine(version, prev, merkle, time, bits, limit=MASK):
    """The same fields with a nonce whose hash does NOT meet bits."""
    head = struct.pack("<i32s32sII", version, prev, merkle, time, bits)
    for nonce in range(1 << 32):
        h = head + struct.pack("<I", nonce)
        if not check_pow(sha256d(h), bits, limit):
            return h
    raise ValueError("every nonce passes")
