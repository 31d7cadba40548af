"""One line of figures from a bench.py JSON line (profiles/scripts_r07/ab_libs.sh): python ab_line.py FILE CONFIG LIBRARY ROUND"""
import json, sys
f, name, lib, r = sys.argv[1:5]
d = json.loads(open(f).read())
s = d.get("single_frame") or {}
print(f"{name:10s} {lib:7s} r{r} ms_per_step {d['ms_per_step']:.4f} (min {d.get('ms_per_step_min')}, max {d.get('ms_per_step_max')}, regions {d.get('timed_regions')}) value {d['value']}"
      + (f" warm {s.get('single_frame_warm_ms')} cold {s.get('single_frame_cold_ms')}" if s else "")
      + f" kernel_ms {(d.get('roofline') or {}).get('kernel_ms')} steps/ray {(d.get('config') or {}).get('steps_per_ray')}", flush=True)
