"""CPU-only: importing dclip_amd makes a fork collect the parent's cyclic garbage first, so that a forked child (DataLoader
worker, multiprocessing manager) never runs the finalizers of objects the parent had already dropped."""
import gc
import os


def test_fork_collects_the_parents_garbage_first():
    import dclip_amd  # noqa: F401
    ran_in = []

    class Node:
        def __del__(self):
            ran_in.append(os.getpid())

    gc.disable()                                   # only the fork hook may collect the cycle below
    try:
        a, b = Node(), Node()
        a.peer, b.peer = b, a
        del a, b
        r, w = os.pipe()
        pid = os.fork()
        if pid == 0:                               # child: report the finalizers that still run here
            os.close(r)
            gc.collect()
            os.write(w, str(len(ran_in) - ran_in.count(os.getppid())).encode())
            os._exit(0)
        os.close(w)
        child_runs = int(os.read(r, 16).decode())
        os.close(r)
        os.waitpid(pid, 0)
    finally:
        gc.enable()
    assert ran_in == [os.getpid()] * 2             # collected in the parent, before the fork
    assert child_runs == 0
