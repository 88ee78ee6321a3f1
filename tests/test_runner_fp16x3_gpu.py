"""The native runner on a net in "fp16x3-layered" mode: test_runner_layered_gpu.py's check with the
mode changed -- the runner sizes its launches by gz_net_wave_rows / gz_net_large_min_rows and launches
through gz_net_forward_segments_ev, which dispatch to the layer-wise trunk with the fp16x3 conv.
breakthroughSmall (6 x 6) on BASELINE config 1's 2 x 64 net, 2 engine threads x 2 pools x 16 games, 8
evaluations per move; pool 0 is replayed through the oracle (oracle/puct_ref.Manager) with the
outputs of the same net's forward -- rows are bit-identical whatever the launch, each board's
exponents being its own -- and every sample the runner emitted for that pool must be identical (at
least 4 of them)."""
import numpy as np
import pytest

from galvanise_zero_amd.nn.desc import BASELINE_CONFIGS
from galvanise_zero_amd.nn.weights import random_weights, to_blob
from puct_harness import Setup, sample_key
from test_runner_fp32_gpu import ROWS, _oracle_conf, _runner_conf, _suffix

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(300)
def test_native_runner_fp16x3_matches_oracle(hip_device):
    from galvanise_zero_amd._native import HipNet
    from galvanise_zero_amd.runner import SelfPlayRunner
    from oracle import puct_ref as P
    desc = BASELINE_CONFIGS[1]["desc"]
    setup = Setup("breakthroughSmall")
    t = setup.transformer
    net = HipNet(desc, hip_device, "fp16x3-layered")
    net.set_weights(to_blob(random_weights(desc, 7921)))
    conf = _runner_conf(8)
    seed, threads, ppt, B, spin = 20251015, 2, 2, 16, 1000
    r = SelfPlayRunner(net, setup.sm, t, conf, device=hip_device, num_threads=threads, pools_per_thread=ppt,
                       batch_size=B, seed=seed, keep_samples=True, spin_yield_playouts=spin,
                       min_launch_rows=32, max_launch_wait_us=2000)
    r.start()
    r.wait_rows(ROWS, timeout_s=60)
    r.stop()
    st = r.stats()
    samples = r.fetch_samples()
    r.close()
    assert st["rows"] > 0, st
    mine = [s for s in samples if int(s["match_identifier"].split("_")[1][1:]) == 0]   # gpu<d>_p<i>_<slot>_<count>

    man = P.Manager(setup.ref_sm, setup.ref_planes, B, P.UniqueStates(setup.ref_planes.hash_mask(), 1000),
                    "t", seed, 0, list(t.policy_dist_count), t.num_rewards, setup.num_prev_states)
    man.start(_oracle_conf(conf, spin))
    pred = (0, [np.zeros(0, np.float32)] * setup.sm.role_count, np.zeros(0, np.float32))
    for _ in range(4000):
        if len(man.samples) >= len(mine):
            break
        buf = man.poll(*pred)
        assert buf is not None
        x = buf.reshape(-1, t.num_channels, t.num_cols, t.num_rows)
        outs = net.forward(x)
        pred = (x.shape[0], outs[:-1], outs[-1])
    n = len(mine)
    assert n >= 4 and len(man.samples) >= n, (n, len(man.samples))
    got = [sample_key(setup, _suffix(s), True) for s in mine]
    exp = [sample_key(setup, _suffix(s), False) for s in man.samples[:n]]
    assert got == exp
    print("fp16x3-layered runner: %d samples of pool 0 identical to the oracle; stats %s" % (n, st))
    net.close()
