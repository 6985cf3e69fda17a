"""CPU: the six option records behave alike, and as each did when it was written out on its own: immutable with the class's name in
the message, repr that evaluates back to an equal record, equality by class and slot values, hash by slot values; and every as_*
maps None, the record itself and its shorthands as documented and refuses everything else by TypeError.

Every expected string below is written out from the classes as they stood in api.py before options.py existed."""
import numpy as np
import pytest

from smalltts_amd import options
from smalltts_amd.options import (Alignment, Delivery, Endpointing, Repair, Takes, Watermark, as_alignment, as_delivery,
                                  as_endpointing, as_repair, as_takes, as_watermark)

# class -> (an instance with no default left alone, its repr, a second, different instance)
CASES = {
    Endpointing: (Endpointing(20.0, 30.0, -70.0, 4, 10.0, 50.0, -20.0, -2.0, 12.0),
                  "Endpointing(frame_ms=20.0, rel_db=30.0, floor_dbfs=-70.0, min_run=4, lead_ms=10.0, tail_ms=50.0, level_dbfs=-20.0, "
                  "peak_dbfs=-2.0, max_gain_db=12.0)", Endpointing()),
    Alignment: (Alignment([3, 1, 1], (7,), [-1, 0]), "Alignment(layers=(1, 3), heads=(7,), steps=(-1, 0))", Alignment()),
    Takes: (Takes(3, (1, 0, 2, 0.5), 0.2, 0.3, 1, 2),
            "Takes(k=3, weights=(1.0, 0.0, 2.0, 0.5), tau_token=0.2, tau_frame=0.3, ctc=1.0, sv=2.0)", Takes(3)),
    Repair: (Repair(2, 0.2, 9, 3), "Repair(rounds=2, tau_token=0.2, max_span=9, margin=3)", Repair()),
    Delivery: (Delivery(16000, "mulaw"), "Delivery(rate=16000, encoding='mulaw')", Delivery()),
    Watermark: (Watermark(7, 0.5), "Watermark(key=7, strength=0.5)", Watermark(7)),
}
DEFAULT_REPRS = {
    Endpointing: "Endpointing(frame_ms=10.0, rel_db=40.0, floor_dbfs=-80.0, min_run=3, lead_ms=30.0, tail_ms=60.0, level_dbfs=None, "
                 "peak_dbfs=-1.0, max_gain_db=20.0)",
    Alignment: "Alignment(layers=None, heads=None, steps=None)",
    Takes: "Takes(k=3, weights=(1.0, 2.0, 1.0, 1.0), tau_token=0.1, tau_frame=0.1, ctc=0.0, sv=0.0)",
    Repair: "Repair(rounds=1, tau_token=0.1, max_span=8, margin=2)",
    Delivery: "Delivery(rate=24000, encoding='f32')",
    Watermark: "Watermark(key=7, strength=0.02)",
}
classes = pytest.mark.parametrize("cls", list(CASES), ids=lambda c: c.__name__)


@classes
def test_setting_and_deleting_raise_with_the_class_in_the_message(cls):
    x = CASES[cls][0]
    for name in (cls.__slots__[0], "no_such_field"):
        with pytest.raises(AttributeError, match=f"^{cls.__name__} is immutable$"):
            setattr(x, name, 1)
        with pytest.raises(AttributeError, match=f"^{cls.__name__} is immutable$"):
            delattr(x, name)
    assert repr(x) == CASES[cls][1]                            # nothing moved
    assert not hasattr(x, "__dict__")


@classes
def test_repr_is_the_slots_in_order_and_evaluates_back(cls):
    x, text, other = CASES[cls]
    assert repr(x) == text and repr(other) == DEFAULT_REPRS[cls]
    for v in (x, other):
        back = eval(repr(v), {cls.__name__: cls})
        assert back == v and back is not v and repr(back) == repr(v)


@classes
def test_equal_values_are_equal_and_hash_equal(cls):
    x, text, other = CASES[cls]
    twin = eval(text, {cls.__name__: cls})
    assert x == twin and not (x != twin) and hash(x) == hash(twin)
    assert hash(x) == hash(tuple(getattr(x, k) for k in cls.__slots__))   # as each class hashed before
    assert x != other and other != x and len({x, twin, other}) == 2
    assert x != text and x != tuple(getattr(x, k) for k in cls.__slots__) and x is not None and not (x == None)  # noqa: E711


def test_unequal_classes_with_equal_slot_values_are_unequal():
    class Other(options._Record):
        __slots__ = ("rate", "encoding")

        def __init__(self, rate, encoding):
            self._set(rate=rate, encoding=encoding)
    d, o = Delivery(8000, "alaw"), Other(8000, "alaw")
    assert [getattr(d, k) for k in d.__slots__] == [getattr(o, k) for k in o.__slots__]
    assert d != o and o != d and not (d == o)
    assert repr(o) == "Other(rate=8000, encoding='alaw')"
    # two records of two slots each whose values coincide
    class Pair(options._Record):
        __slots__ = ("key", "strength")

        def __init__(self, key, strength):
            self._set(key=key, strength=strength)
    assert Watermark(7, 0.5) != Pair(7, 0.5) and Pair(7, 0.5) != Watermark(7, 0.5) and Pair(7, 0.5) == Pair(7, 0.5)


def test_piece_keeps_its_own_repr_and_compares_by_identity():
    p = options.Piece([1, 2, 3], 1, np.zeros((4, 64), np.float32), 9)
    q = options.Piece([1, 2, 3], 1, np.zeros((4, 64), np.float32), 9)
    assert repr(p) == "Piece(tokens=3, prefix_len=1, frames=4, seed=9)"
    assert p == p and p != q and hash(p) != hash(q) and len({p, q}) == 2
    with pytest.raises(AttributeError, match="^Piece is immutable$"):
        p.seed = 1
    with pytest.raises(AttributeError, match="^Piece is immutable$"):
        del p.seed


# as_* -> (the function, its class, accepted shorthand -> the record it means, refused values, the message up to the type's name)
COERCIONS = {
    "trim": (as_endpointing, Endpointing, [(True, Endpointing())], [1, 0, 1.0, "yes", (1, 2), np.bool_(True)],
             "trim must be None, a bool or an Endpointing, got "),
    "align": (as_alignment, Alignment, [(True, Alignment())], [1, 0, 1.0, "yes", (1, 2), np.bool_(True)],
              "align must be None, a bool or an Alignment, got "),
    "takes": (as_takes, Takes, [(4, Takes(4)), (np.int64(2), Takes(2))], [True, False, 2.0, "2", (2, 3), [2]],
              "takes must be None, an int or a Takes, got "),
    "repair": (as_repair, Repair, [(2, Repair(2)), (np.int32(3), Repair(3))], [True, False, 2.0, "2", (2, 3)],
               "repair must be None, an int or a Repair, got "),
    "deliver": (as_delivery, Delivery, [(8000, Delivery(8000)), (np.int64(16000), Delivery(16000)), ((8000, "alaw"), Delivery(8000, "alaw")),
                                        ([48000, "pcm16"], Delivery(48000, "pcm16"))],
                [True, False, 8000.0, "8000", (8000,), (8000, "alaw", 1)], "deliver must be None, a Delivery, a rate or a (rate, encoding) pair, got "),
    "watermark": (as_watermark, Watermark, [(7, Watermark(7)), (np.uint64(2 ** 63), Watermark(2 ** 63)), ((7, 0.5), Watermark(7, 0.5)),
                                            ([7, 1], Watermark(7, 1.0))],
                  [True, False, 7.0, "7", (7,), (7, 0.5, 1)], "watermark must be None, a Watermark, a key or a (key, strength) pair, got "),
}


@pytest.mark.parametrize("name", list(COERCIONS))
def test_as_functions_map_none_the_record_and_its_shorthands(name):
    fn, cls, accepted, _refused, _msg = COERCIONS[name]
    assert fn(None) is None
    x = CASES[cls][0]
    assert fn(x) is x
    for short, want in accepted:
        got = fn(short)
        assert type(got) is cls and got == want, (short, got)
    if name in ("trim", "align"):
        assert fn(False) is None


@pytest.mark.parametrize("name", list(COERCIONS))
def test_as_functions_refuse_everything_else_by_type_error(name):
    fn, _cls, _accepted, refused, msg = COERCIONS[name]
    for bad in refused + ["text", object()]:
        with pytest.raises(TypeError) as e:
            fn(bad)
        assert str(e.value) == msg + type(bad).__name__, (bad, str(e.value))
    if name not in ("trim", "align"):                          # a bool where an int is expected
        with pytest.raises(TypeError) as e:
            fn(True)
        assert str(e.value) == msg + "bool"


def test_a_pair_reaches_the_class_and_its_own_refusals():
    with pytest.raises(TypeError, match="^Delivery: rate must be an integer, got bool$"):
        as_delivery((True, "f32"))
    with pytest.raises(ValueError, match="^Delivery: encoding must be one of "):
        as_delivery((8000, "mp3"))
    with pytest.raises(TypeError, match="^Watermark: strength must be a number, got str$"):
        as_watermark((7, "0.5"))
    with pytest.raises(ValueError, match=r"^Watermark: strength must be in \[0, 1\], got nan$"):
        as_watermark((7, float("nan")))
    with pytest.raises(ValueError, match=r"^Takes: k must lie in \[1, 16\], got 17$"):
        as_takes(17)
    with pytest.raises(ValueError, match=r"^Repair: rounds must lie in \[1, 4\], got 0$"):
        as_repair(0)
