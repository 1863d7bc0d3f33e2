"""TrustedRows and DevicePartition on the host side of the engine mirror, without a device: the two config keys parse, and the
combinations DevicePartition cannot work in are refused before the context is looked at."""
import ctypes as C
import json

import pytest

from bloomsearch_amd import host as Hst

FULL = dict(DeviceIngest=True, DeviceIngestStream=True, TrustedRows=True, DevicePartition=True, PartitionField="tenant")


def open_rc(**config):
    L = Hst.lib()
    cfg = json.dumps(config).encode()
    h = C.c_void_p()
    rc = L.bse_open(cfg, len(cfg), None, C.byref(h))
    assert not h.value
    return rc


def without(key, **more):
    cfg = {k: v for k, v in FULL.items() if k != key}
    cfg.update(more)
    return cfg


def test_the_two_keys_parse():
    assert open_rc(**FULL) == -1                                   # BSH_E_INVALID: the config was fine, the context is NULL
    assert open_rc(TrustedRows=True) == -1 and open_rc(TrustedRows=False) == -1
    assert open_rc(TrustedRows=True, PartitionField="tenant", DeviceIngest=True, DeviceIngestStream=True) == -1
    assert open_rc(DevicePartition=False) == -1
    assert open_rc(**dict(FULL, PartitionField="n" * 64, MinMaxIndexes=["ts", "v"])) == -1


@pytest.mark.parametrize("cfg", [without("DeviceIngestStream"), without("DeviceIngest"), without("TrustedRows"), without("TrustedRows", TrustedRows=False),
                                 without("PartitionField"), without("PartitionField", PartitionField=""), without("PartitionField", PartitionField="n" * 65),
                                 dict(DevicePartition=True)],
                         ids=["no stream", "no device ingest", "no trust", "trust false", "no field", "empty field", "65-byte field", "alone"])
def test_the_refused_combinations_are_refused(cfg):
    assert open_rc(**cfg) == -101                                  # BSE_E_INVALID_CONFIG, before the NULL context is looked at
