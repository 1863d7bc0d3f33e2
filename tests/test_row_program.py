"""The row matchers' one program evaluator (no GPU): tests/row_program_check.cpp, built with plain g++ against
bloomsearch_amd/csrc/host/row_program.hpp, compared with a recursive evaluation of the expression TREE written here from the opcode
contract: a program is the postfix form of a binary tree of TERM c / TRUE / FALSE leaves under AND2 / OR2 nodes (opcode in the top four
bits: 0, 3, 4, 1, 2), at most 64 values are ever on the stack, and the empty program is the nil expression, which matches."""
import os
import subprocess

import numpy as np
import pytest


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERM, AND2, OR2, TRUE, FALSE = 0, 1, 2, 3, 4
REGISTER, WORDS = 0, 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("row_program") / "row_program_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "row_program_check.cpp")], check=True, timeout=300)
    return exe


class Answers:
    def __init__(self, words):
        self.w, self.at = words, 0

    def take(self, n=None):
        if n is None:
            self.at += 1
            return int(self.w[self.at - 1])
        self.at += n
        return [int(x) for x in self.w[self.at - n: self.at]]

    def done(self):
        return self.at == len(self.w)


def run_driver(exe, tmp_path, cases):
    words = np.concatenate([np.asarray([len(cases)], dtype="<u8")] + [np.asarray(c, dtype="<u8") for c in cases])
    words.tofile(tmp_path / "cases.bin")
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return Answers(np.fromfile(tmp_path / "answers.bin", dtype="<u8"))


# ---- the contract, restated: trees as ("t", c) / True / False / ("and", l, r) / ("or", l, r) ----
def tree_value(node, flag):
    if isinstance(node, bool):
        return node
    if node[0] == "t":
        return flag(node[1])
    left, right = tree_value(node[1], flag), tree_value(node[2], flag)
    return (left and right) if node[0] == "and" else (left or right)


def postfix(node, out):
    if isinstance(node, bool):
        out.append((TRUE if node else FALSE) << 28)
    elif node[0] == "t":
        out.append(TERM << 28 | node[1])
    else:
        postfix(node[1], out)
        postfix(node[2], out)
        out.append((AND2 if node[0] == "and" else OR2) << 28)
    return out


def stack_need(node):
    """the most values on the stack while the node's postfix form runs"""
    if isinstance(node, bool) or node[0] == "t":
        return 1
    return max(stack_need(node[1]), 1 + stack_need(node[2]))


def terms_in_order(node):
    if isinstance(node, bool):
        return []
    if node[0] == "t":
        return [node[1]]
    return terms_in_order(node[1]) + terms_in_order(node[2])


def random_leaf(rng, n_terms):
    pick = rng.integers(0, 10)
    return bool(pick & 1) if pick < 2 else ("t", int(rng.integers(0, n_terms)))


def random_tree(rng, budget, n_terms):
    """a tree whose postfix form needs at most `budget` stack values: a right spine of random length (a right child runs with one
    more value under it), small random trees or leaves to its left, so that deep stacks are as common as shallow ones"""
    if budget <= 1 or rng.random() < 0.25:
        return random_leaf(rng, n_terms)
    spine = int(rng.integers(1, budget))
    node = random_tree(rng, min(budget - spine, 4), n_terms)
    for under in range(spine - 1, -1, -1):                                             # values on the stack under this node
        left = random_leaf(rng, n_terms) if rng.random() < 0.8 else random_tree(rng, min(budget - under, 4), n_terms)
        node = ("and" if rng.random() < 0.5 else "or", left, node)
    return node


def chain(leaves, ops):
    """leaves[0] op (leaves[1] op (leaves[2] op ...)): the right-leaning chain, stack need = len(leaves)"""
    node = leaves[-1]
    for leaf, op in zip(reversed(leaves[:-1]), reversed(ops)):
        node = (op, leaf, node)
    return node


def flag_of(words):
    return lambda c: bool(words[c >> 6] >> (c & 63) & 1)


def case(reader, trees, words):
    """the trees' programs behind each other, one range each (a None tree: the empty range), one set of flag words"""
    prog, ranges = [], []
    for t in trees:
        j0 = len(prog)
        if t is not None:
            postfix(t, prog)
        ranges += [j0, len(prog)]
    return [reader, len(prog)] + prog + [len(trees)] + ranges + [len(words)] + list(words)


def fetches(trees):
    """what a reader that keeps the last word fetches: one word per change of c >> 6 in program order, across the ranges"""
    n, cur = 0, None
    for t in trees:
        for c in terms_in_order(t) if t is not None else []:
            if c >> 6 != cur:
                n, cur = n + 1, c >> 6
    return n


def test_random_programs_up_to_depth_64_over_one_register_word(driver, tmp_path):
    rng = np.random.default_rng(64)
    cases, want, needs = [], [], set()
    for _ in range(300):
        budget = int(rng.choice([1, 2, 3, 8, 33, 64]))
        trees = [random_tree(rng, budget, 64) for _ in range(4)]
        needs |= {stack_need(t) for t in trees}
        word = int(rng.integers(0, 1 << 64, dtype=np.uint64)) & [0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF, 0][int(rng.integers(0, 3))]
        cases.append(case(REGISTER, trees, [word]))
        want += [tree_value(t, flag_of([word])) for t in trees]
    assert max(needs) == 64 and len(needs) > 40 and 1 in needs and True in want and False in want
    a = run_driver(driver, tmp_path, cases)
    assert a.take(len(want)) == want and a.done()


def test_the_right_leaning_depth_64_chain(driver, tmp_path):
    """64 leaves, then 63 operators: every level of the one-bit stack is in use, the verdict hangs on the leaf pushed FIRST (the
    stack's top bit) as on the one pushed last"""
    leaves = [("t", c) for c in range(64)]
    all_and, all_or = chain(leaves, ["and"] * 63), chain(leaves, ["or"] * 63)
    mixed = chain(leaves, ["and" if i % 2 else "or" for i in range(63)])
    assert stack_need(all_and) == 64 and len(postfix(all_and, [])) == 127
    ones = (1 << 64) - 1
    words = [ones, ones ^ 1, ones ^ 1 << 63, ones ^ 1 << 31, 0, 1, 1 << 63, 1 << 32, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA]
    trees = [all_and, all_or, mixed]
    a = run_driver(driver, tmp_path, [case(REGISTER, trees, [w]) for w in words])
    want = [tree_value(t, flag_of([w])) for w in words for t in trees]
    assert want[:6] == [True, True, True, False, True, True] and want[12:15] == [False, False, False] and want[15:17] == [False, True]
    assert a.take(len(want)) == want and a.done()


def test_the_empty_program_matches_and_constants_alone(driver, tmp_path):
    trees = [None, True, False, None, ("t", 0), ("and", True, False), ("or", False, True), None]
    a = run_driver(driver, tmp_path, [case(REGISTER, trees, [0]), case(WORDS, trees, [0, 0]), case(REGISTER, [None], [0])])
    want = [True, True, False, True, False, False, True, True]
    assert a.take(8) == want and a.take(8) == want and a.take() == 1 and a.take() == 1 and a.done()   # one word fetched: TERM 0's


@pytest.mark.parametrize("bit", [63, 64, 127, 128])
def test_terms_on_both_sides_of_a_word_boundary_read_by_a_reader_that_serves_words(driver, tmp_path, bit):
    rng = np.random.default_rng(bit)
    cases, want = [], []
    for words in ([0, 0, 0, 0], [1 << 63, 0, 0, 0], [0, 1, 0, 0], [0, 1 << 63, 0, 0], [0, 0, 1, 0], [(1 << 64) - 1] * 4,
                  [int(x) for x in rng.integers(0, 1 << 64, size=4, dtype=np.uint64)]):
        lone = ("t", bit)
        pair = ("and", ("t", bit), ("or", ("t", bit - 1), ("t", bit + 1)))                # both neighbours: one of them lies in another word
        back = chain([("t", c) for c in (bit, bit ^ 64, bit, 255, 0, bit)], ["or", "and", "or", "and", "or"])   # the kept word changes back and forth
        trees = [lone, pair, None, back, lone] + [random_tree(rng, 16, 256) for _ in range(6)]
        cases.append(case(WORDS, trees, words))
        want += [tree_value(t, flag_of(words)) if t is not None else True for t in trees] + [fetches(trees)]
    a = run_driver(driver, tmp_path, cases)
    assert a.take(len(want)) == want and a.done()
    assert True in want and False in want
