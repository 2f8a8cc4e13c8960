"""CPU: oakgpu_set_move_carry_dry refuses a null context (its range check needs a context: tests/test_gpu_queue_frames.py), and the
Python face has the setter."""


def test_set_move_carry_dry_refuses_a_null_context():
    import __graft_entry__ as g
    g.build()
    from oak_amd import _lib
    lib = _lib.load()
    for below in (0, 8, 64, 65, -1):
        assert lib.oakgpu_set_move_carry_dry(None, below) != 0, below
    assert b"oakgpu_set_move_carry_dry" in lib.oakgpu_last_error()


def test_context_has_the_setter():
    from oak_amd.engine import Context
    assert callable(Context.set_move_carry_dry)
