"""The oracle of the alignment summaries (include/pw_txsum.h) in pure Python: ``str.count``, ``find`` and ``rfind`` -- the
operations ``pipeline.map_queries`` and ``Alignment.truncate_to_match`` apply to transcript strings on the host."""
FIELDS = ('n_match', 'n_subst', 'n_ins', 'n_del', 'n_gaps', 'first_match', 'last_match', 'head_origin', 'head_mutant',
          'tail_origin', 'tail_mutant', 'flags')
NONE = (0, 0, 0, 0, 0, -1, -1, 0, 0, 0, 0, 0)          # a pair without a summarised transcript
ST_TRACED, ST_EMPTY, ST_PANICK, ST_BADPATH = 1, 2, 4, 8


def summarize(tx, status=ST_TRACED):
    """The 12 fields of ``pw_tx_summary`` for transcript ``tx`` (a ``str`` or None) of a pair with the ``PW_ST_*`` bits
    ``status``: NONE without a transcript, an empty one, or a record the header excludes."""
    if not tx or not status & ST_TRACED or status & (ST_EMPTY | ST_PANICK | ST_BADPATH):
        return NONE
    gaps = sum(1 for k in range(len(tx)) if tx[k] in 'ID' and (k == 0 or tx[k - 1] != tx[k]))
    first, last = tx.find('M'), tx.rfind('M')
    ho = hm = to = tm = 0
    if first >= 0:
        head, tail = tx[:first], tx[last + 1:]
        ho, hm = head.count('S') + head.count('D'), head.count('S') + head.count('I')
        to, tm = tail.count('S') + tail.count('D'), tail.count('S') + tail.count('I')
    return (tx.count('M'), tx.count('S'), tx.count('I'), tx.count('D'), gaps, first, last, ho, hm, to, tm, 1)


def as_tuples(records):
    """A SUMMARY_DTYPE array as a list of tuples in FIELDS order."""
    return [tuple(int(r[f]) for f in FIELDS) for r in records]


def assert_equal(records, expected, what=''):
    got = as_tuples(records)
    assert len(got) == len(expected), (what, len(got), len(expected))
    for k, (g, e) in enumerate(zip(got, expected)):
        assert g == e, (what, k, dict(zip(FIELDS, g)), dict(zip(FIELDS, e)))
