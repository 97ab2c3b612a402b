// rf_comm_local.cpp -- the LOCAL transport of the frame exchange (rf_transport.hpp): a TEST transport, chosen with RF_COMM_TRANSPORT=local when the id is made.
//
// The same exchange -- the same transfer list, the same staging offsets, the same un-tile -- with every send / receive pair replaced by a device-to-device copy between
// the buffers of N communicators that live in ONE process, one host thread per rank.  RCCL refuses two ranks on one device, and the boxes this is developed on have one
// GPU: without this, the gather and kUntile had only ever executed with one owner (world 1: every tile `own`, or every tile staging in loop-back).  With it, worlds
// 2 / 3 / 4 / 8 run on one GPU: the root's receives land at rankFirstTile[peer] of its staging area, kUntile picks own / staging per tile from tileOwner / tileSlot,
// and the image must equal the single-rank one bit for bit (tests/test_gpu_parity.py: test_local_transport_gather_*).  What it does NOT exercise: RCCL itself and xGMI.
//
// Semantics mirror a group of point-to-point operations: a send is matched with the receive the peer posts for it, in posting order per (source, destination); the
// receiver's stream waits for the sender's stream (an event recorded behind the sender's frame kernels), copies, and the sender's stream waits for the copy before
// anything queued behind the exchange may touch the buffer again.  Host side a rank posts all its sends, then performs its receives (each waits for its send to be
// posted), then waits until its sends have been taken -- dead-lock free for the gather (and for loop-back).  A peer that never arrives is an error after
// RF_COMM_TIMEOUT_S, as with RCCL.
#include "rf_transport.hpp"

#include "rf_hip_host.hpp"

#include <algorithm>
#include <array>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <random>

namespace rf
{
namespace
{
constexpr char kLocalMagic[8] = {'R', 'F', 'L', 'O', 'C', 'A', 'L', '1'};

struct LocalPost
{
    const void* src = nullptr;
    size_t      bytes = 0;
    int         srcDevice = 0;
    hipEvent_t  ready = nullptr;    // recorded on the sender's stream behind everything queued before the exchange
    hipEvent_t  consumed = nullptr; // recorded on the receiver's stream behind its copy (set when `taken`)
    bool        taken = false;
};

struct LocalFabric
{
    uint32_t                world = 0;
    std::mutex              mutex;
    std::condition_variable cv;
    std::map<std::pair<uint32_t, uint32_t>, std::deque<std::shared_ptr<LocalPost>>> mail; // (source, destination) -> sends not yet received, oldest first
    std::vector<hipEvent_t> freeEvents, allEvents;
    // allReduceMax: a generation barrier
    uint64_t generation = 0;
    uint32_t arrived = 0;
    double   running = 0.0, result = 0.0;

    hipEvent_t takeEvent() // (mutex held)
    {
        if (!freeEvents.empty())
        {
            hipEvent_t e = freeEvents.back();
            freeEvents.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        RF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        allEvents.push_back(e);
        return e;
    }
    ~LocalFabric()
    {
        for (hipEvent_t e : allEvents) (void)hipEventDestroy(e);
    }
};

std::mutex                                                              gFabricMutex;
std::map<std::array<uint8_t, kCommIdBytes>, std::weak_ptr<LocalFabric>> gFabrics;

// (not collective: a rank's peers are waited for in the exchange itself)
std::shared_ptr<LocalFabric> attachFabric(const uint8_t id[kCommIdBytes], uint32_t world)
{
    std::array<uint8_t, kCommIdBytes> key;
    std::memcpy(key.data(), id, kCommIdBytes);
    std::lock_guard<std::mutex> lock(gFabricMutex);
    std::shared_ptr<LocalFabric> f = gFabrics[key].lock();
    if (!f)
    {
        f = std::make_shared<LocalFabric>();
        f->world = world;
        gFabrics[key] = f;
    }
    if (f->world != world) throw std::runtime_error("local transport: the ranks of one id disagree about the world size");
    for (auto it = gFabrics.begin(); it != gFabrics.end();) it = it->second.expired() ? gFabrics.erase(it) : std::next(it);
    return f;
}

class LocalTransport final : public Transport
{
    std::shared_ptr<LocalFabric> mFabric;
    uint32_t                     mRank, mWorld;
    int                          mDevice;

    template<typename Ready>
    void waitFor(std::unique_lock<std::mutex>& lock, Ready&& ready, const char* what) const
    {
        const double timeout = commTimeoutSeconds();
        if (timeout <= 0.0) return mFabric->cv.wait(lock, ready);
        if (!mFabric->cv.wait_for(lock, std::chrono::duration<double>(timeout), ready))
            throw std::runtime_error(std::string("local transport: ") + what + " did not happen within " + std::to_string(static_cast<int>(timeout)) + " s on rank " +
                                     std::to_string(mRank) + " (a peer is missing or disagrees about frame size / root)");
    }

public:
    LocalTransport(const uint8_t id[kCommIdBytes], uint32_t rank, uint32_t world, int device) : mFabric(attachFabric(id, world)), mRank(rank), mWorld(world), mDevice(device) {}

    bool isLocal() const override { return true; }
    void info(uint32_t& count, uint32_t& userRank, int& device) const override { count = mWorld, userRank = mRank, device = mDevice; } // (no RCCL communicator behind it)

    void exchange(const std::vector<Transfer>& transfers, hipStream_t stream) override
    {
        LocalFabric&                            f = *mFabric;
        std::vector<std::shared_ptr<LocalPost>> mine;
        for (const Transfer& op : transfers) // 1. post every send
        {
            if (!op.isSend) continue;
            auto post = std::make_shared<LocalPost>();
            post->src = op.from;
            post->bytes = op.words * sizeof(uint32_t);
            post->srcDevice = mDevice;
            {
                std::lock_guard<std::mutex> lock(f.mutex);
                post->ready = f.takeEvent();
            }
            RF_HIP(hipEventRecord(post->ready, stream));
            {
                std::lock_guard<std::mutex> lock(f.mutex);
                f.mail[{mRank, op.peer}].push_back(post);
            }
            f.cv.notify_all();
            mine.push_back(post);
        }
        for (const Transfer& op : transfers) // 2. every receive: wait for the peer's send, copy behind it
        {
            if (op.isSend) continue;
            std::shared_ptr<LocalPost> post;
            {
                std::unique_lock<std::mutex> lock(f.mutex);
                auto&                        box = f.mail[{op.peer, mRank}];
                waitFor(lock, [&] { return !box.empty(); }, "a peer's send");
                post = box.front();
                box.pop_front();
                post->consumed = f.takeEvent();
            }
            if (post->bytes != op.words * sizeof(uint32_t)) // (a plane's tiles or a shard's counts: each operation has its own size)
                throw std::runtime_error("local transport: rank " + std::to_string(op.peer) + " sends " + std::to_string(post->bytes) + " bytes, rank " + std::to_string(mRank) + " expects " +
                                         std::to_string(op.words * sizeof(uint32_t)) + " (the ranks disagree about the frame)");
            RF_HIP(hipStreamWaitEvent(stream, post->ready, 0));
            RF_HIP(hipMemcpyAsync(op.to, post->src, post->bytes, hipMemcpyDeviceToDevice, stream));
            RF_HIP(hipEventRecord(post->consumed, stream));
            {
                std::lock_guard<std::mutex> lock(f.mutex);
                post->taken = true;
            }
            f.cv.notify_all();
        }
        for (const std::shared_ptr<LocalPost>& post : mine) // 3. my sends: the buffer is mine again once the receiver's copy has run
        {
            {
                std::unique_lock<std::mutex> lock(f.mutex);
                waitFor(lock, [&] { return post->taken; }, "the root's receive");
            }
            RF_HIP(hipStreamWaitEvent(stream, post->consumed, 0));
            std::lock_guard<std::mutex> lock(f.mutex);
            f.freeEvents.push_back(post->ready);
            f.freeEvents.push_back(post->consumed);
        }
    }

    // a generation barrier over the fabric's ranks (host side; the caller's stream is drained first, as the RCCL path's read-back does)
    double allReduceMax(double value, hipStream_t stream) override
    {
        RF_HIP(hipStreamSynchronize(stream));
        LocalFabric&                 f = *mFabric;
        std::unique_lock<std::mutex> lock(f.mutex);
        const uint64_t               gen = f.generation;
        f.running = f.arrived == 0 ? value : std::max(f.running, value);
        if (++f.arrived == f.world)
        {
            f.result = f.running;
            f.arrived = 0;
            ++f.generation;
            f.cv.notify_all();
            return f.result;
        }
        const double timeout = commTimeoutSeconds();
        const auto   released = [&] { return f.generation != gen; };
        if (timeout > 0.0)
        {
            if (!f.cv.wait_for(lock, std::chrono::duration<double>(timeout), released)) throw std::runtime_error("local transport: all-reduce timed out on rank " + std::to_string(mRank));
        }
        else f.cv.wait(lock, released);
        return f.result;
    }
};
} // namespace

bool makeLocalUniqueId(uint8_t out[kCommIdBytes])
{
    const char* v = std::getenv("RF_COMM_TRANSPORT");
    if (v == nullptr || std::strcmp(v, "local") != 0) return false;
    // the magic prefix + 120 random bytes
    std::memcpy(out, kLocalMagic, sizeof kLocalMagic);
    std::random_device rd;
    for (uint32_t i = sizeof kLocalMagic; i < kCommIdBytes; ++i) out[i] = static_cast<uint8_t>(rd());
    return true;
}

std::unique_ptr<Transport> makeLocalTransport(const uint8_t id[kCommIdBytes], uint32_t rank, uint32_t worldSize, int device)
{
    if (std::memcmp(id, kLocalMagic, sizeof kLocalMagic) != 0) return nullptr;
    return std::make_unique<LocalTransport>(id, rank, worldSize, device);
}
} // namespace rf
