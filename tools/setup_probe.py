"""C4 registrations from device-resident clouds, timed by phase (the bench's step, its registration()):
set_model_device, set_scene_device, run(30).  Medians over REPS registrations after a warm-up."""
import os, sys, time, json
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "iterative-closest-point_amd"))
import icp_amd
n = 1 << 20
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
m, p = icp_amd.synthetic_pair(n, seed=42)
dm = torch.from_numpy(m).to("cuda:0"); dp = torch.from_numpy(p).to("cuda:0")
torch.cuda.synchronize()
s = torch.cuda.current_stream(dm.device).cuda_stream
rows = []
with icp_amd.Context(0) as ctx:
    for k in range(reps + 5):
        t0 = time.perf_counter()
        ctx.set_model_device(dm.data_ptr(), n, stream=s)
        t1 = time.perf_counter()
        ctx.set_scene_device(dp.data_ptr(), n, n, stream=s)
        t2 = time.perf_counter()
        ctx.run(30, -1.0)
        t3 = time.perf_counter()
        if k >= 5:
            rows.append((t1 - t0, t2 - t1, t3 - t2, t3 - t0))
a = np.array(rows) * 1e6
med = np.median(a, axis=0)
print("probe", json.dumps({"env": {k: v for k, v in os.environ.items() if k.startswith("ICP_")},
                           "set_model_us": round(med[0], 1), "set_scene_us": round(med[1], 1), "run_us": round(med[2], 1),
                           "total_us": round(med[3], 1), "total_min_us": round(a[:, 3].min(), 1)}))
