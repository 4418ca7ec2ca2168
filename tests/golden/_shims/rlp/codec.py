def _prefix(n, base):
    if n < 56:
        return bytes([base + n])
    be = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([base + 55 + len(be)]) + be


def encode_raw(item):
    if isinstance(item, (bytes, bytearray)):
        item = bytes(item)
        return item if len(item) == 1 and item[0] < 0x80 else _prefix(len(item), 0x80) + item
    if isinstance(item, str):
        return encode_raw(item.encode())
    if isinstance(item, int):
        return encode_raw(item.to_bytes((item.bit_length() + 7) // 8, "big"))
    body = b"".join(encode_raw(x) for x in item)
    return _prefix(len(body), 0xC0) + body


def encode(obj, sedes=None, **kw):
    return encode_raw(sedes.serialize(obj) if sedes is not None else obj)


def _item(data, pos):
    b0 = data[pos]
    if b0 < 0x80:
        return data[pos:pos + 1], pos + 1
    is_list = b0 >= 0xC0
    v = b0 - (0xC0 if is_list else 0x80)
    start = pos + 1
    if v >= 56:
        start += v - 55
        v = int.from_bytes(data[pos + 1:start], "big")
    end = start + v
    if end > len(data):
        raise ValueError("RLP item runs past its buffer")
    if not is_list:
        return data[start:end], end
    out = []
    while start < end:
        x, start = _item(data, start)
        out.append(x)
    return out, end


def decode(data, sedes=None, **kw):
    obj, end = _item(bytes(data), 0)
    if end != len(data):
        raise ValueError("trailing bytes after the RLP item")
    return sedes.deserialize(obj) if sedes is not None else obj
