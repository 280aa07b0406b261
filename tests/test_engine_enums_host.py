"""The parsers of openhevc_amd/engine.py that take a name of a table or its number: what each returns for a known name and a known
number, and the ValueError of an unknown name and of a number outside the table, word for word.  Three of them (formats, resize filters,
the reformat modes) let any number pass, as the library refuses it with its own message.  No GPU, no library call."""
import pytest

from openhevc_amd import engine as E


def _reformat(**kw):
    return lambda v: object.__new__(E.Engine).pics_reformat([], **{k: (v if x is None else x) for k, x in kw.items()})


def _warp_mode(v):
    return E.warp_matrix([65536, 0, 0, 0, 65536, 0], v)[0]


def _warp_filter(v):
    e = object.__new__(E.Engine)
    e._params = {}
    with pytest.raises(E.EngineError, match="picture 1 was not allocated"):   # what follows the parsers: no picture 1
        e.pics_warp([1], [65536, 0, 0, 0, 65536, 0], (8, 8), filter=v)


# the parser, (a name, its number), a number it takes, an unknown name and its text, a number outside the table and its text (None: it passes)
CASES = {
    "conv_format": (E.conv_format, ("rgb_planar", 2), 4, "nv21", "unknown format 'nv21': one of ['planar', 'rgb', 'rgb_planar', 'rgba', 'semiplanar']", 9, None),
    "resize_filter": (E.resize_filter, ("bicubic", 1), 0, "lanczos", "unknown filter 'lanczos': one of ['bicubic', 'bilinear']", 7, None),
    "orient_code": (E.orient_code, ("rot90", 5), 7, "rot45", "unknown orientation 'rot45': one of ['antitranspose', 'hflip', 'identity', 'rot180', "
                    "'rot270', 'rot90', 'transpose', 'vflip']", 8, "orientation 8: 0 .. 7"),
    "deint_mode": (E.deint_mode, ("lowpass5", 2), 3, "weave", "unknown deinterlacing mode 'weave': one of ['adaptive', 'blend', 'bob', 'lowpass5']",
                   4, "deinterlacing mode 4: 0 .. 3"),
    "filter_mode": (E.filter_mode, ("median", 2), 0, "blur", "unknown filter mode 'blur': one of ['convolve', 'median', 'temporal', 'unsharp']",
                    -1, "filter mode -1: 0 .. 3"),
    "warp_mode": (_warp_mode, ("perspective", 1), 0, "shear", "unknown mode 'shear': one of ['affine', 'perspective']", 2, "mode 2: one of [0, 1]"),
}
# parsers that are reached only through a wrapper, which returns nothing of them: the texts alone
REFUSALS = {
    "reformat_depth": (_reformat(depth=None), "round", 1, "floor", "unknown depth mode 'floor': one of ['dither', 'round']", 5, None),
    "reformat_down": (_reformat(down=None), "point", 1, "cubic", "unknown down filter 'cubic': one of ['linear', 'nearest', 'point']", 5, None),
    "reformat_up": (_reformat(up=None), "nearest", 0, "cubic", "unknown up filter 'cubic': one of ['linear', 'nearest', 'point']", -3, None),
    "warp_filter": (_warp_filter, "bicubic", 0, "lanczos", "unknown filter 'lanczos': one of ['bicubic', 'bilinear', 'nearest']", 3,
                    "filter 3: one of [0, 1, 2]"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_known_names_and_numbers(name):
    parse, (word, number), other = CASES[name][:3]
    assert parse(word) == number and parse(number) == number and parse(other) == other


@pytest.mark.parametrize("name", sorted(CASES) + sorted(REFUSALS))
def test_refusals_word_for_word(name):
    parse, known, number, bad_word, word_text, bad_number, number_text = (CASES.get(name) or REFUSALS[name])
    if name in REFUSALS:
        parse(known), parse(number)                           # neither raises a ValueError
    with pytest.raises(ValueError) as err:
        parse(bad_word)
    assert str(err.value) == word_text
    if number_text is None:
        assert name in REFUSALS or parse(bad_number) == bad_number
        if name in REFUSALS:
            parse(bad_number)
    else:
        with pytest.raises(ValueError) as err:
            parse(bad_number)
        assert str(err.value) == number_text
