"""Shared by test_lp_model_host.py and test_gpu_polytope_fidelity.py: the linear programs of
tests/golden/polytope_fidelity.npz rebuilt without a GPU.  The fixture names its POVM; the n-qubit tensor is the
repeated np.kron of the one-qubit table, which generate_measurement_matrix reproduces bit for bit on the device."""
import numpy as np
from conftest import load_golden


def host_povm(name, n_qubits):
    from quantpy_amd.measurements import _ONE_QUBIT

    table = _ONE_QUBIT[name]()
    table = table[None] if table.ndim == 2 else table
    out = table
    for _ in range(n_qubits - 1):
        out = np.kron(out, table)
    return out


def golden():
    return load_golden("polytope_fidelity")


def process_case(g, name):
    """(A, b (n_points, M), c, deltas, frequencies) of a process case, from the fixture's arrays alone."""
    from quantpy_amd.tomography.polytopes.fidelity import process_programs

    n = int(g[name + "/n_qubits"])
    dim = 4**n
    povm = host_povm(str(g[name + "/povm"]), n)
    A, b, deltas, freq = process_programs(g[name + "/states_matrix"], povm, g[name + "/shots"], g[name + "/counts"],
                                          int(g[name + "/n_points"]))
    c = g[name + "/target_bloch"].reshape(dim, dim)[:, 1:].ravel()
    return A, b, c, deltas, freq


def state_case(g, name):
    """(A, b, c, deltas, frequencies) of a state case through StateFidelityInterval.programs() (host code)."""
    import quantpy_amd as qp
    from quantpy_amd.tomography.polytopes import StateFidelityInterval

    n = int(g[name + "/n_qubits"])
    tmg = qp.StateTomograph(qp.qobj.fully_mixed(n))
    tmg.povm_matrix = host_povm(str(g[name + "/povm"]), n)
    tmg.results = g[name + "/counts"]
    interval = StateFidelityInterval(tmg, n_points=int(g[name + "/n_points"]), target_state=qp.Qobj(g[name + "/target_bloch"]))
    return interval.programs()


def case_programs(g, name):
    return process_case(g, name) if name in list(g["process_cases"]) else state_case(g, name)


def all_cases():
    g = golden()
    return list(g["process_cases"]) + list(g["state_cases"])
