class BigEndianInt:
    def __init__(self, length=None):
        self.length = length

    def serialize(self, obj):
        raw = obj.to_bytes((obj.bit_length() + 7) // 8, "big")
        return raw if self.length is None else raw.rjust(self.length, b"\0")

    def deserialize(self, serial):
        return int.from_bytes(serial, "big")


class Binary:
    def __init__(self, min_length=None, max_length=None, allow_empty=False):
        self.min_length, self.max_length, self.allow_empty = min_length, max_length, allow_empty

    @classmethod
    def fixed_length(cls, n, allow_empty=False):
        return cls(n, n, allow_empty)

    def serialize(self, obj):
        return bytes(obj)

    def deserialize(self, serial):
        return bytes(serial)


big_endian_int = BigEndianInt()
binary = Binary()
