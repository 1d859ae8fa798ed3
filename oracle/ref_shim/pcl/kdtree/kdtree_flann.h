/* oracle/ref_shim -- stand-in for <pcl/kdtree/kdtree_flann.h> (TEST INFRASTRUCTURE, NOT PRODUCT CODE).
 *
 * The five headers under oracle/ref_shim/pcl let the reference's own initRegistrationKSS.hpp and
 * registrationMeasure.hpp compile untouched into oracle/_ref/kss_ref_front (oracle/Makefile.ref), so that the
 * compiler -- not a reading -- settles their loop trip counts, overloads, expression order and comparisons.
 * This is the only one of the five with behaviour.
 *
 * nearestKSearch is an exact search by exhaustion: the k nearest cloud points in ascending (d2, index) order,
 * k clipped to the cloud size and the two output vectors resized to it, as pcl::KdTreeFLANN does.
 *
 * CAVEAT.  The distance arithmetic is OUR READING of FLANN's L2_Simple<float> functor, which PCL's kd-tree
 * instantiates: result = 0; then result += diff * diff for x, y, z in that order, every operation in float and
 * none fused.  FLANN is not part of the reference tree, so this is the one thing a comparison against the
 * compiled binary does not make independent of the hand that wrote oracle/kss_oracle.c.  FLANN's order among
 * equidistant points depends on its tree traversal; here the lowest index wins, and only distances (never
 * indices) reach the reference's results on these paths. */
#pragma once
#include <cstddef>
#include <vector>

#include <pcl/point_cloud.h>

namespace pcl {

template <typename PointT>
class KdTreeFLANN {
public:
    typedef typename PointCloud<PointT>::ConstPtr PointCloudConstPtr;

    KdTreeFLANN() {}

    void setInputCloud(const PointCloudConstPtr &cloud) { input_ = cloud; }

    int nearestKSearch(const PointT &point, int k, std::vector<int> &k_indices,
                       std::vector<float> &k_sqr_distances) const {
        const std::size_t n = input_ ? input_->points.size() : 0;
        if (k < 0) k = 0;
        if ((std::size_t)k > n) k = (int)n;
        k_indices.resize(k);
        k_sqr_distances.resize(k);
        if (k == 0) return 0;
        int have = 0;
        for (std::size_t j = 0; j < n; j++) {
            const PointT &q = input_->points[j];
            float r = 0.0f, d;
            d = point.x - q.x; r += d * d;
            d = point.y - q.y; r += d * d;
            d = point.z - q.z; r += d * d;
            /* insertion into the sorted prefix; a later index never overtakes an equal distance */
            if (have == k && !(r < k_sqr_distances[k - 1])) continue;
            int pos = have < k ? have++ : k - 1;
            while (pos > 0 && r < k_sqr_distances[pos - 1]) {
                k_sqr_distances[pos] = k_sqr_distances[pos - 1];
                k_indices[pos] = k_indices[pos - 1];
                pos--;
            }
            k_sqr_distances[pos] = r;
            k_indices[pos] = (int)j;
        }
        return k;
    }

private:
    PointCloudConstPtr input_;
};

}  // namespace pcl
