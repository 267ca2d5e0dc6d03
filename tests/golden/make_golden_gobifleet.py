"""A second real dataset for the fleet tests: the first 400 lines of the
reference's simulator trace (scheduler/BaGTI/datasets/simulator/
energy_latency_16_scheduling.csv, 2,400 lines), data only, copied as they are.
load_energy_latency_data drops the first line (utils.py:59's header quirk), so
it gives 399 samples, with another max_ips than the framework trace's.
Writes tests/golden/energy_latency_16_scheduling_simulator400.csv (about 150 KB).
"""
import os

SRC = "/root/reference/scheduler/BaGTI/datasets/simulator/energy_latency_16_scheduling.csv"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "energy_latency_16_scheduling_simulator400.csv")

if __name__ == "__main__":
    with open(SRC) as f:
        lines = f.readlines()[:400]
    with open(OUT, "w") as f:
        f.writelines(lines)
    print(OUT, len(lines), "lines", os.path.getsize(OUT), "bytes")
