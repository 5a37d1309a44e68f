"""A schedule simulation of k_match_both over bench.py's workload, on the CPU:
how long the launch runs after the ticket is empty, and what lanes that
advance faster in that phase would save.  A MODEL - tests/hw/lane_tail.py is
the measurement (profiles/lane_tail_timeline.txt holds both).

Assumptions:
  * rounds per block from tests/model_match_lane_multi.py at depth 1, over the
    12 bench inputs, tiled `tiles` times in stream order;
  * `lanes` lanes draw blocks from the front of the list, `windows` window
    wavefronts from its back, a window block taking 0.4 us x its rounds;
  * every busy lane advances min(1 / 1.5 us, 2.05e10 / busy lanes) rounds a
    second: the latency of a round, or its share of the memory system's
    random-access rate;
  * with a speed-up k, the latency of a round is 1.5 us / k from the moment
    the ticket is empty (the memory system's rate stays what it is).
usage: python tests/hw/lane_tail_model.py [tiles] [lanes] [windows]"""
import heapq
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import model_match_lane_multi as M  # noqa: E402
import oracle_lib as O  # noqa: E402

LATENCY = 1.5e-6      # seconds a round, memory idle
RATE = 2.05e10        # rounds a second, memory saturated
WINDOW = 0.4e-6       # seconds a round's worth of a window wavefront's block


def block_rounds():
    """rounds of every block of one corpus round, in stream order"""
    out = []
    for _, data in O.corpus_round():
        for at in range(0, len(data), 65536):
            blk = data[at:at + 65536]
            out.append(M.lane_tokens(blk, 1)[1] if len(blk) >= 17 else 0)
    return out


def simulate(rounds, tiles, lanes, windows, speedup=1.0):
    """(launch s, ticket empty at s, s spent below saturation)"""
    blocks = rounds * tiles
    front, back = 0, len(blocks)          # the two-ended ticket
    t = v = 0.0     # time; rounds a lane that was busy all along has done
    busy = []       # heap of v at which a lane finishes its block
    wins = []       # heap of t at which a window wavefront finishes
    for _ in range(min(lanes, back)):
        heapq.heappush(busy, v + blocks[front])
        front += 1
    for _ in range(windows):
        if front < back:
            back -= 1
            heapq.heappush(wins, t + WINDOW * blocks[back])
    empty_at, unsat = None, 0.0
    while busy or wins:
        lat = LATENCY / (speedup if front >= back else 1.0)
        rate = min(1.0 / lat, RATE / len(busy)) if busy else 0.0
        t_lane = t + (busy[0] - v) / rate if busy else float("inf")
        t_win = wins[0] if wins else float("inf")
        t_next = min(t_lane, t_win)
        if busy and rate < RATE / len(busy) * (1 - 1e-12) or not busy:
            unsat += t_next - t
        v += (t_next - t) * rate
        t = t_next
        if t_lane <= t_win:
            heapq.heappop(busy)
            if front < back:
                heapq.heappush(busy, v + blocks[front])
                front += 1
        else:
            heapq.heappop(wins)
            if front < back:
                back -= 1
                heapq.heappush(wins, t + WINDOW * blocks[back])
        if empty_at is None and front >= back:
            empty_at = t
    return t, empty_at, unsat


def main():
    tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 2934
    lanes = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    windows = int(sys.argv[3]) if len(sys.argv) > 3 else 512
    rounds = block_rounds()
    print(f"# {len(rounds)} blocks a corpus round, {sum(rounds)} rounds; "
          f"x {tiles} tiles, {lanes} lanes, {windows} window wavefronts")
    base = None
    for k in (1.0, 1.22, 1.5):
        t, empty, unsat = simulate(rounds, tiles, lanes, windows, k)
        base = base or t
        print(f"tail speed-up {k:4.2f}: launch {t * 1e3:6.1f} ms, ticket "
              f"empty at {empty * 1e3:5.1f} ms, below saturation "
              f"{unsat * 1e3:5.1f} ms, saves {(base - t) * 1e3:4.1f} ms")


if __name__ == "__main__":
    main()
