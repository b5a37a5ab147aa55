"""The numpy restatement of the device generator (tests/rng_oracle.py) on its own: Philox's known
answers, the Feistel permutation as a bijection, and its uniformity.  No GPU."""
import numpy as np
import pytest

import rng_oracle as O

# (counter, key) -> words: Random123's known answers for philox4x32-10
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,words", KAT)
def test_philox_known_answers(counter, key, words):
    got = O.philox4x32_10(np.array(counter, np.uint64), np.array(key, np.uint64))
    assert [int(x) for x in got] == list(words)


@pytest.mark.parametrize("n", [1, 2, 3, 128, 150, 384, 1024, 1025, 16000])
def test_feistel_is_a_bijection(n):
    for draw, policy, array in ((0, 0, 0), (5, 3, 7)):
        v = O.permutation(0x1234_5678_9ABC_DEF0, draw, policy, array, n)
        assert v.dtype == np.int32 and v.shape == (n,)
        assert np.array_equal(np.sort(v), np.arange(n))


def test_feistel_keys_differ():
    a = O.permutation(11, 0, 0, 0, 384)
    assert not np.array_equal(a, O.permutation(12, 0, 0, 0, 384))   # seed
    assert not np.array_equal(a, O.permutation(11, 1, 0, 0, 384))   # draw
    assert not np.array_equal(a, O.permutation(11, 0, 1, 0, 384))   # policy
    assert not np.array_equal(a, O.permutation(11, 0, 0, 1, 384))   # array
    assert not np.array_equal(a, O.permutation(11, 1 << 32, 0, 0, 384))   # the draw's high word


def test_feistel_uniformity():
    """n = 384 over 4,000 draws of one stream: the 12 x 12 table (position // 32, value // 32) of all
    draws against equal cells.  Every draw is a permutation, so the table's margins are exact and
    chi^2 has (12 - 1)^2 = 121 degrees of freedom; z = (chi^2 - 121) / sqrt(242) must stay <= 5."""
    n, draws, bins = 384, 4000, 12
    v = O.permutation(20260101, np.arange(draws), 0, 0, n)
    assert v.shape == (draws, n)
    pos = np.broadcast_to(np.arange(n) // (n // bins), v.shape)
    table = np.zeros((bins, bins))
    np.add.at(table, (pos.ravel(), (v // (n // bins)).ravel()), 1.0)
    expect = draws * n / bins ** 2
    chi2 = ((table - expect) ** 2 / expect).sum()
    dof = (bins - 1) ** 2
    z = (chi2 - dof) / np.sqrt(2 * dof)
    print(f"chi2 {chi2:.1f} dof {dof} z {z:.2f}")
    assert z <= 5.0


def test_noise_restatement_moments():
    """The fp64 noise of the restatement is standard normal: mean, variance and fourth moment over
    2^18 values within 5 standard errors (1 / sqrt n, sqrt(2 / n), sqrt(96 / n))."""
    z = O.noise(7, 0, 64, 512, 4, 2).ravel()
    n = z.size
    assert abs(z.mean()) <= 5 / np.sqrt(n)
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    assert abs((z ** 4).mean() - 3) <= 5 * np.sqrt(96 / n)


def test_noise_position_and_shape_invariance():
    a = O.noise(3, 0, 7, 9, 4, 2)
    assert np.array_equal(a[3:], O.noise(3, 3, 4, 9, 4, 2))        # the position is the absolute step
    assert np.array_equal(a[:, :5], O.noise(3, 0, 7, 5, 4, 2))     # env e does not depend on N
    assert np.array_equal(a.reshape(7, 9, 8), O.noise(3, 0, 7, 9, 1, 8).reshape(7, 9, 8))   # flat components
