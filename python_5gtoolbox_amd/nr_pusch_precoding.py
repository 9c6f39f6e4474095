"""Drop-in for py5gphy/nr_pusch/nr_pusch_precoding.py: the codebook precoding matrices W of
38.211 Tables 6.3.1.5-1 (one layer, two antenna ports) and 6.3.1.5-4 (two layers, two ports,
transform precoding disabled), as host tables (RS_info["precoding_matrix"] of pusch_dmrs_LS_est)."""
import numpy as np

_R2 = 2 ** -0.5
# (layers, antenna ports) -> (scale, one entry per TPMI index: the matrix written row by row)
_CODEBOOK = {
    (1, 2): (_R2, ((1, 0), (0, 1), (1, 1), (1, -1), (1, 1j), (1, -1j))),
    (2, 2): (None, ((_R2, 0, 0, _R2), (.5, .5, .5, -.5), (.5, .5, .5j, -.5j))),
}


def get_precoding_matrix(num_of_layers, nNrOfAntennaPorts, nPMI):
    """complex64 W (ports, layers) of TPMI index nPMI; [1] for one layer on one port; None for a
    combination without a table here (as the reference, nr_pusch_precoding.py:6-32)."""
    if (num_of_layers, nNrOfAntennaPorts) == (1, 1):
        return np.ones(1, np.complex64)
    entry = _CODEBOOK.get((num_of_layers, nNrOfAntennaPorts))
    if entry is None:
        return None
    scale, rows = entry
    assert nPMI < len(rows), f"nPMI {nPMI}: the table has indices 0..{len(rows) - 1}"
    W = np.array(rows[nPMI], np.complex64).reshape(nNrOfAntennaPorts, num_of_layers)
    return W if scale is None else W * np.float32(scale)
