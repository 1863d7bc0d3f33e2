"""Named rows for the keyed ingest's partition rule, each with its STATED text and whether the device decides it (tests/
partition_restatement.py must agree: test_partition_shapes.py).  Shared by the CPU tests, the sanitizer programs and the GPU tests."""
from dataclasses import dataclass

from tests.partition_restatement import MAX_KEY

NAME64 = "n" * 64


@dataclass(frozen=True)
class Shape:
    name: str
    field: str
    row: bytes
    text: bytes          # the partition text (what the host decides for every row)
    undecided: bool      # the device hands the row back


def S(name, field, row, text, undecided=False):
    return Shape(name, field, row.encode("utf-8") if isinstance(row, str) else row, text.encode("utf-8") if isinstance(text, str) else text, undecided)


def _value_shapes():
    big = "123456789012345678901234567890"
    vals = [("string", '"alpha"', "alpha"), ("empty_string", '""', ""), ("zero", "0", "0"), ("minus_zero", "-0", "-0"), ("one_point_zero", "1.0", "1.0"),
            ("exponent", "1e5", "1e5"), ("exponent_signed", "-2.5E+3", "-2.5E+3"), ("thirty_digits", big, big), ("true", "true", "true"),
            ("false", "false", "false"), ("null", "null", ""), ("object", "{}", ""), ("array", "[]", ""),
            ("nested_object_with_name", '{"p":"inner","q":[{"p":1}]}', ""), ("array_of_strings", '["p","x"]', "")]
    return [S("value_" + n, "p", '{"a":1,"p":%s,"z":"t"}' % v, t) for n, v, t in vals]


def _length_shapes():
    out = []
    for n in (0, 1, MAX_KEY - 1, MAX_KEY, MAX_KEY + 1):
        out.append(S("string_of_%d" % n, "p", '{"p":"%s","z":1}' % ("s" * n), "s" * n, n > MAX_KEY))
    for n in (MAX_KEY - 1, MAX_KEY, MAX_KEY + 1):
        out.append(S("number_of_%d" % n, "p", '{"p":%s}' % ("7" * n), "7" * n, n > MAX_KEY))
    out.append(S("long_string_with_late_backslash", "p", '{"p":"%s\\\\n"}' % ("s" * 200), "s" * 200 + "\\n", True))
    return out


SHAPES = [
    S("member_first", "p", '{"p":"a","x":1,"y":"t"}', "a"),
    S("member_middle", "p", '{"x":1,"p":"b","y":"t"}', "b"),
    S("member_last", "p", '{"x":1,"y":"t","p":"c"}', "c"),
    S("member_absent", "p", '{"x":1,"y":"t"}', ""),
    S("empty_object", "p", "{}", ""),
    S("duplicate_first_wins", "p", '{"p":"first","p":"second"}', "first"),
    S("duplicate_first_is_null", "p", '{"p":null,"p":"second"}', ""),
    S("duplicate_second_escaped", "p", '{"p":"first","p":"sec\\\\ond"}', "first"),
    S("same_key_one_level_down", "p", '{"o":{"p":"inner"},"q":1}', ""),
    S("same_key_down_then_top", "p", '{"o":{"p":"inner"},"p":"outer"}', "outer"),
    S("same_key_in_array", "p", '{"o":[{"p":"inner"}],"p":"outer"}', "outer"),
    S("ts_against_t_and_tsx", "ts", '{"t":"no","tsx":"no","ts":"yes"}', "yes"),
    S("ts_only_t_and_tsx", "ts", '{"t":"no","tsx":"no"}', ""),
    S("name64_against_key65", NAME64, '{"%s":"long","%s":"right"}' % (NAME64 + "n", NAME64), "right"),
    S("name64_only_key65", NAME64, '{"%s":"long"}' % (NAME64 + "n"), ""),
    S("empty_key_in_row", "p", '{"":"e","p":"x"}', "x"),
    S("raw_utf8", "p", '{"p":"grüße-日本-🎉","z":1}', "grüße-日本-🎉"),
    S("raw_utf8_key_elsewhere", "p", '{"ключ":"v","p":"x"}', "x"),
    S("backslash_in_value", "p", '{"p":"a\\\\nb"}', "a\\nb", True),
    S("escaped_quote_in_value", "p", '{"p":"a\\"b"}', 'a"b', True),
    S("unicode_escape_in_value", "p", '{"p":"\\u0041"}', "A", True),
    S("escaped_key_before", "p", '{"\\u0070x":1,"p":"v"}', "v", True),
    S("escaped_key_is_the_member", "p", '{"\\u0070":"hidden","p":"v"}', "hidden", True),
    S("escaped_key_after", "p", '{"p":"v","\\u0070":"later"}', "v"),
    S("escaped_key_no_member", "p", '{"a\\\\b":1,"c":2}', "", True),
    S("escaped_key_nested_only", "p", '{"o":{"a\\\\b":1},"p":"v"}', "v"),
    S("escaped_nested_value_before", "p", '{"o":"x\\\\\\"y","p":"v"}', "v"),
    S("structure_inside_strings", "p", '{"a":"{}[]:,","b":"x\\"p\\":\\"no\\"","c":["}","{\\"p\\":1"],"p":"yes"}', "yes"),
    S("string_ends_with_escaped_backslash", "p", '{"a":"tail\\\\\\\\","p":"yes"}', "yes"),
    S("white_space_everywhere", "p", ' \t{ "a" : 1 ,\n "p" \r:  "w s" , "z" : [ 1 , 2 ] } \n', "w s"),
    S("white_space_number", "p", '{ "p" :\t-12.50\n, "z":1}', "-12.50"),
    S("white_space_true_last", "p", '{"z":1, "p" : true }', "true"),
    S("number_last_no_space", "p", '{"z":1,"p":42}', "42"),
    S("string_5", "p", '{"p":"5"}', "5"),
    S("number_5", "p", '{"p":5}', "5"),
    S("value_contains_name", "p", '{"a":"p","b":"\\"p\\"","p":"v"}', "v"),
    S("deep_nesting_before", "p", '{"a":' + "[" * 40 + "]" * 40 + ',"p":"deep"}', "deep"),
] + _value_shapes() + _length_shapes()

assert len({s.name for s in SHAPES}) == len(SHAPES)


def at_every_alignment(shapes=SHAPES):
    """[(shape or None, row)]: every shape's row at each of the eight start alignments of a packed batch (filler rows of one field's
    partition "" in between, None)"""
    out, at = [], 0
    for s in shapes:
        for a in range(8):
            pad = (a - at - 2) % 8 + 2                         # a filler of >= 2 bytes that ends at alignment a
            out.append((None, b"{" + b" " * (pad - 2) + b"}"))
            at = (at + pad) % 8
            assert at == a
            out.append((s, s.row))
            at = (at + len(s.row)) % 8
    return out
