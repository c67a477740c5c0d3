"""ImplicitFactorizationModel.recommend without a GPU: the method exists and refuses bad arguments
before any device work (checked on a bare object that holds only the model's shape)."""
import numpy as np
import pytest
import scipy.sparse as sp

from recommendation_gans_amd.implicit import ImplicitFactorizationModel

U, I = 20, 9


def bare():
    m = ImplicitFactorizationModel.__new__(ImplicitFactorizationModel)
    m._num_users, m._num_items, m._kind = U, I, "mf"
    return m


@pytest.mark.parametrize("kw", [
    dict(user_ids=[0, U]), dict(user_ids=[-1]), dict(user_ids=np.array([3, 2 ** 40])),
    dict(user_ids=[1], k=0), dict(user_ids=[1], k=-3), dict(user_ids=[1], k=I + 1), dict(user_ids=[1], k=33),
    dict(user_ids=[1], exclude=sp.csr_matrix((U, I + 1))), dict(user_ids=[1], exclude=sp.csr_matrix((U + 1, I))),
])
def test_bad_arguments_raise_value_error(kw):
    with pytest.raises(ValueError):
        bare().recommend(**kw)


def test_k_is_capped_at_32_whatever_the_item_count():
    m = bare()
    m._num_items = 1000
    with pytest.raises(ValueError):
        m.recommend([1], k=33)


def test_no_users_is_an_empty_result():
    ids = bare().recommend(np.zeros(0, np.int64), k=5)
    assert ids.shape == (0, 5) and ids.dtype == np.int64
    ids, sc = bare().recommend([], k=3, exclude=sp.csr_matrix((U, I)), return_scores=True)
    assert ids.shape == sc.shape == (0, 3) and sc.dtype == np.float32
