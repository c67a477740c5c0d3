"""Interaction sets (spotlight/interactions.py:38-178 of the reference).

Same constructor, attributes, ``__len__``, ``tocoo``/``tocsr`` and ``has_key``
(which, as in the reference, compares the RAW rating stored at construction
with 1: ``interactions.py:159-160``).  Validation raises the reference's
ValueError messages (``interactions.py:136-158``).

``Interactions.to_sequence`` and ``SequenceInteractions`` (additive; upstream Spotlight's
semantics, which the reference's copy dropped): each user's items in timestamp order, cut into
windows from the END of the history, left-padded with 0 -- the input of
``sequence.ImplicitSequenceModel``."""
import numpy as np
import scipy.sparse as sp


class Interactions:
    def __init__(self, user_ids, item_ids, ratings=None, timestamps=None, weights=None,
                 num_users=None, num_items=None):
        self.num_users = num_users or int(user_ids.max() + 1)
        self.num_items = num_items or int(item_ids.max() + 1)
        self.user_ids = user_ids
        self.item_ids = item_ids
        self.ratings = ratings
        self.timestamps = timestamps
        self.weights = weights
        self.shape = (num_users, num_items)
        self.csr_matrix = self.tocsr()      # raw ratings, kept for has_key
        self._check()

    def __repr__(self):
        return "<Interactions dataset ({} users x {} items x {} interactions)>".format(
            self.num_users, self.num_items, len(self))

    def __len__(self):
        return len(self.user_ids)

    def _check(self):
        if self.user_ids.max() >= self.num_users:
            raise ValueError("Maximum user id greater than declared number of users.")
        if self.item_ids.max() >= self.num_items:
            raise ValueError("Maximum item id greater than declared number of items.")
        n = len(self.user_ids)
        for name, value in (("item IDs", self.item_ids), ("ratings", self.ratings),
                            ("timestamps", self.timestamps), ("weights", self.weights)):
            if value is not None and len(value) != n:
                raise ValueError("Invalid {} dimensions: length must be equal to number of "
                                 "interactions".format(name))

    def has_key(self, user, item):
        return self.csr_matrix[user, item] == 1

    def tocoo(self):
        data = self.ratings if self.ratings is not None else np.ones(len(self))
        return sp.coo_matrix((data, (self.user_ids, self.item_ids)), shape=(self.num_users, self.num_items))

    def tocsr(self):
        return self.tocoo().tocsr()

    def to_sequence(self, max_sequence_length=10, min_sequence_length=None, step_size=None):
        """Each user's history, sorted by timestamp, as windows of ``max_sequence_length`` items:
        the first window ends at the user's last item, the next ``step_size`` items earlier
        (default: ``max_sequence_length``, windows that do not overlap), until the history is used
        up; a window shorter than the maximum is padded with 0 on the LEFT.  With
        ``min_sequence_length`` a window holding fewer items than that is dropped.  Item id 0 is
        the padding id and is refused in the input."""
        if self.timestamps is None:
            raise ValueError("Cannot convert to sequences, timestamps not available.")
        if max_sequence_length < 1 or (step_size is not None and step_size < 1):
            raise ValueError("max_sequence_length and step_size must be at least 1")
        if len(self.item_ids) and (np.asarray(self.item_ids) == 0).any():
            raise ValueError("0 is used as an item id, conflicting with the sequence padding value.")
        step = max_sequence_length if step_size is None else int(step_size)
        order = np.lexsort((self.timestamps, self.user_ids))
        users, items = np.asarray(self.user_ids)[order], np.asarray(self.item_ids)[order]
        uniq, start, count = np.unique(users, return_index=True, return_counts=True)
        rows, row_users = [], []
        for u, s0, n in zip(uniq, start, count):
            for end in range(int(n), 0, -step):
                window = items[s0 + max(end - max_sequence_length, 0):s0 + end]
                row = np.zeros(max_sequence_length, dtype=np.int32)
                row[max_sequence_length - len(window):] = window
                rows.append(row)
                row_users.append(u)
        sequences = np.stack(rows) if rows else np.zeros((0, max_sequence_length), dtype=np.int32)
        row_users = np.asarray(row_users, dtype=np.int32)
        if min_sequence_length is not None:
            if not 1 <= min_sequence_length <= max_sequence_length:
                raise ValueError("min_sequence_length must be in [1, max_sequence_length]")
            keep = sequences[:, -min_sequence_length] != 0
            sequences, row_users = sequences[keep], row_users[keep]
        return SequenceInteractions(sequences, user_ids=row_users, num_items=self.num_items)


class SequenceInteractions:
    """Left-padded item sequences [num_sequences, max_sequence_length] (0 is padding), the user
    each came from, and the number of items."""

    def __init__(self, sequences, user_ids=None, num_items=None):
        sequences = np.asarray(sequences)
        if sequences.ndim != 2:
            raise ValueError("sequences must be [num_sequences, max_sequence_length]")
        if user_ids is not None and len(user_ids) != len(sequences):
            raise ValueError("user_ids must hold one id per sequence")
        if sequences.size and sequences.min() < 0:
            raise ValueError("negative item id in sequences")
        self.sequences = sequences
        self.user_ids = user_ids
        self.max_sequence_length = sequences.shape[1]
        self.num_items = int(num_items) if num_items is not None else int(sequences.max() + 1 if sequences.size else 1)
        if sequences.size and sequences.max() >= self.num_items:
            raise ValueError("Maximum item id greater than declared number of items.")

    def __repr__(self):
        return "<Sequence interactions dataset ({} sequences x {} sequence length)>".format(*self.sequences.shape)

    def __len__(self):
        return len(self.sequences)
